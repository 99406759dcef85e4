"""The filter_anime hook of the speech_anime surface on the MI355X (where the reference's identity hook _filter_anime sits,
model.py:405-406,420): the returned, written and exported rows are sdfa_amd.tfilter's result on the unfiltered rows, clip by
clip; without a spec nothing changes."""
import os

import numpy as np
import pytest
import torch

from speech_anime.hparams import configure
from speech_anime.api import build_model
from speech_anime.datasets import DatasetSlidingWindow
from sdfa_amd import synth, tfilter

pytestmark = pytest.mark.gpu
SR = 16000


@pytest.fixture(scope="module")
def model(synth_sd):
    hp = configure(dict(mode="evaluate", custom_hparams="dgrad"))
    hp.audio.set_key("sample_rate", SR)
    DatasetSlidingWindow.hparams = None
    return build_model(hp, synth_sd["dgrad"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _filtered(spec, animes):
    rows = torch.from_numpy(np.ascontiguousarray(animes, np.float32)).cuda().reshape(len(animes), -1)
    return tfilter.apply(spec, rows).cpu().numpy().reshape(animes.shape)


def test_generate_animation_is_the_filtered_unfiltered_call(model):
    pcm = synth.make_pcm(0, 2 * SR)
    ts0, a0, _ = model.generate_animation(pcm, "m1", 0, 0)
    a0 = a0.copy()
    spec = "bilateral:1,0.05,3"
    ts1, a1, others = model.generate_animation(pcm, "m1", 0, 0, filter_anime=spec)
    assert ts1 == ts0 and a1.shape == a0.shape == (len(ts0), 9976, 9) and a1.dtype == np.float32
    want = tfilter.bilateral(torch.from_numpy(a0).cuda(), 1.0, 0.05, 3).cpu().numpy()
    assert np.array_equal(_bits(a1), _bits(want))
    assert not np.array_equal(_bits(a1), _bits(a0))                      # it did something
    assert others["inputs"].shape == (len(ts0), 3, 128, 64)
    ts2, a2, _ = model.generate_animation(pcm, "m1", 0, 0)               # and the default is as before
    assert ts2 == ts0 and np.array_equal(_bits(a2), _bits(a0))
    with pytest.raises(ValueError, match="filter"):
        model.generate_animation(pcm, "m1", 0, 0, filter_anime="median:3")


def test_custom_dataset_class_route_filters_too(model):
    pcm = synth.make_pcm(3, SR)

    class Same(DatasetSlidingWindow):
        pass
    _, a0, _ = model.generate_animation(pcm, "m1", 0, 0, dataset_class=Same)
    _, a1, _ = model.generate_animation(pcm, "m1", 0, 0, dataset_class=Same, filter_anime="gaussian:1")
    assert np.array_equal(_bits(a1), _bits(_filtered("gaussian:1", a0)))


def test_batch_filters_each_clip_alone(model):
    clips = [synth.make_pcm(1, 2 * SR), synth.make_pcm(2, SR)]
    plain = [(ts, a.copy()) for ts, a, _ in model.generate_animation_batch(clips, "m1")]
    outs = model.generate_animation_batch(clips, "m1", filter_anime="gaussian:1")
    assert len(outs) == 2
    for (ts0, a0), (ts1, a1, _) in zip(plain, outs):
        assert ts1 == ts0
        assert np.array_equal(_bits(a1), _bits(_filtered("gaussian:1", a0)))
    # the last frames of clip 0 do not see clip 1: filtering the concatenation would differ there
    cat = _filtered("gaussian:1", np.concatenate([plain[0][1], plain[1][1]]))
    assert not np.array_equal(_bits(cat[len(plain[0][0]) - 1]), _bits(outs[0][1][-1]))


def test_speaker_sweep_over_the_cached_signal_is_filtered(model):
    pcm = synth.make_pcm(4, SR)
    model.generate_animation(pcm, "m1", 0, 0)                            # fills the signal cache
    assert model._signal_cache is not None
    _, a0, _ = model.generate_animation(pcm, "m2", 0, 0)
    a0 = a0.copy()
    _, a1, _ = model.generate_animation(pcm, "m2", 0, 0, filter_anime="bilateral:1,0.05,3")
    assert model._signal_cache is not None                               # both calls were served from it
    assert np.array_equal(_bits(a1), _bits(_filtered("bilateral:1,0.05,3", a0)))


def test_evaluate_writes_the_filtered_track(tmp_path, model):
    from scipy.io import wavfile
    from speech_anime import viewer
    viewer.clear_template()
    wav = tmp_path / "clip.wav"
    wavfile.write(str(wav), SR, (synth.make_pcm(6, SR) * 32767).astype(np.int16))
    sources = {"test": [(str(wav), "speaker=m1")]}
    plain = model.evaluate(sources, output_dir=str(tmp_path / "plain"), export_mesh_frames=True)
    filt = model.evaluate(sources, output_dir=str(tmp_path / "filt"), export_mesh_frames=True, filter_anime="gaussian:1.5")
    (_, ts0, a0), (_, ts1, a1) = plain[0], filt[0]
    want = _filtered("gaussian:1.5", a0)
    assert ts1 == ts0 and np.array_equal(_bits(a1), _bits(want))
    saved = np.load(tmp_path / "filt" / "clip" / "dgrad_3d.npy")
    assert np.array_equal(_bits(saved), _bits(want))
    assert np.array_equal(_bits(np.load(tmp_path / "plain" / "clip" / "dgrad_3d.npy")), _bits(a0))
    # the exported frames are blended from the filtered rows: what the plain export makes of the filtered track
    names = sorted(n for n in os.listdir(tmp_path / "filt" / "clip") if n.endswith("_dgrad.npy"))
    assert names == sorted(n for n in os.listdir(tmp_path / "plain" / "clip") if n.endswith("_dgrad.npy")) and names
    from sdfa_amd.seek import SeekPlan
    plan = SeekPlan([ts0], model.hp.anime.fps, device="cuda:0")
    rows = plan.rows(torch.from_numpy(want).cuda().reshape(len(ts0), -1)).cpu().numpy()
    for i in (0, len(names) // 2, len(names) - 1):
        assert np.array_equal(_bits(np.load(tmp_path / "filt" / "clip" / names[i])), _bits(rows[i].reshape(-1, 9)))
    assert getattr(model, "_filtered_rows", None) is None               # nothing stays pinned on the device
