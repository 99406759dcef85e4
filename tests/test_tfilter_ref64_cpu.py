"""The temporal track filters without a device: the float64 restatements (tests/tfilter_ref64.py) against scipy and the
reference's BilateralFilter1D (tests/golden/track_filter.npz), the Gaussian taps, the filter-spec grammar, the PLY reader of
the dataset step, and through the built library the exported symbols, the ABI version and every refusal, none of which
launches anything."""
import json
import os
import re

import numpy as np
import pytest

import tfilter_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = (1, 2, 3, 4, 5, 8, 9, 10, 33, 100)
SIGMAS = (0.1, 0.5, 1, 2, 8)            # radii 0, 2, 4, 8, 32


def _signal(F, W, seed):
    rs = np.random.RandomState(seed)
    return (rs.normal(0, 1e-3, (F, W)) * (1 + 10 * (rs.uniform(size=(1, W)) < 0.1))).astype(np.float32)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gaussian_ref_is_scipy_bitwise(sigma):
    from scipy.ndimage import gaussian_filter1d
    assert len(R.gaussian_taps_ref(sigma)) // 2 == {0.1: 0, 0.5: 2, 1: 4, 2: 8, 8: 32}[sigma]
    for F in FRAMES:
        x = _signal(F, 257, 7 * F)
        want = gaussian_filter1d(x, sigma, axis=0)
        got = R.gaussian_ref(x, sigma)
        assert want.dtype == got.dtype == np.float32
        assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), (sigma, F)
    frames = [row for row in _signal(9, 33, 1)]                  # a list of 1-D arrays, as preload.py:819 passes
    assert np.array_equal(gaussian_filter1d(frames, sigma=sigma, axis=0), R.gaussian_ref(frames, sigma))


def test_clips_are_filtered_independently_by_the_ref():
    x = _signal(12, 5, 3)
    whole = R.gaussian_ref(x, 1, clip_frame_off=[0, 5, 6, 12])
    for a, b in ((0, 5), (5, 6), (6, 12)):
        assert np.array_equal(whole[a:b], R.gaussian_ref(x[a:b], 1))
    assert np.array_equal(R.bilateral_ref(x, radius=3, clip_frame_off=[0, 5, 12])[5:], R.bilateral_ref(x[5:], radius=3))


@pytest.mark.parametrize("sigma,truncate", [(0.1, 4.0), (0.5, 4.0), (1, 4.0), (1.0, 3.0), (2, 4.0), (2.5, 2.0), (8, 4.0)])
def test_gaussian_taps_are_scipys_kernel(sigma, truncate):
    from scipy.ndimage import correlate1d, gaussian_filter1d
    from sdfa_amd import tfilter
    taps = tfilter.gaussian_taps(sigma, truncate)
    assert taps.dtype == np.float64 and taps.size == 2 * int(truncate * float(sigma) + 0.5) + 1
    assert taps.tobytes() == taps[::-1].tobytes()
    assert taps.tobytes() == R.gaussian_taps_ref(sigma, truncate).tobytes()
    x = _signal(40, 17, 5).astype(np.float64)
    assert np.array_equal(correlate1d(x, taps, axis=0, mode="reflect"), gaussian_filter1d(x, sigma, axis=0, truncate=truncate))
    for bad in (0.0, -1.0, float("nan"), float("inf"), 9.0):     # 9 * 4 + 0.5 -> radius 36
        with pytest.raises(ValueError):
            tfilter.gaussian_taps(bad)


def _bilateral_cases(golden):
    z = golden["track_filter"]
    f0 = 0
    for pi, ai, F in z["bilateral_index"]:
        ds, rs, r = z["bilateral_params"][pi]
        yield (float(ds), float(rs), int(r)), z["bilateral_signal"][f0:f0 + F], z["bilateral_out64"][f0:f0 + F], z["bilateral_out32"][f0:f0 + F]
        f0 += F
    assert f0 == len(z["bilateral_signal"])


def test_bilateral_ref_is_the_references_filter(golden):
    with open(os.path.join(ROOT, "tests", "golden", "META_track_filter.json")) as fp:
        meta = json.load(fp)
    n, worst64, worst32 = 0, 0.0, 0.0
    for (ds, rs, r), x, out64, out32 in _bilateral_cases(golden):
        assert x.dtype == np.float32 and x.shape[1] == 7
        amp = float(np.abs(x).max())
        got = R.bilateral_ref64(x, ds, rs, r)
        worst64 = max(worst64, float(np.abs(got - out64).max()) / amp)
        worst32 = max(worst32, float(np.abs(R.bilateral_ref(x, ds, rs, r).astype(np.float64) - out32).max()) / amp)
        n += 1
    print(f"{n} cases: |ref64 - reference on float64| / max|x| = {worst64:.2e}; |float32(ref64) - reference on float32| / max|x| = {worst32:.2e} "
          f"(recorded float32-run error {meta['bilateral_f32_vs_f64_rel']:.2e})")
    assert n == 2 * 2 * 6
    assert worst64 <= 1e-14
    assert worst32 <= 2 * meta["bilateral_f32_vs_f64_rel"]


def test_parse_filter_grammar_and_refusals():
    from sdfa_amd.tfilter import parse_filter
    assert parse_filter("gaussian:1") == ("gaussian", {"sigma": 1.0})
    assert parse_filter(" Gaussian : 0.75 ".replace(" : ", ":")) == ("gaussian", {"sigma": 0.75})
    assert parse_filter("bilateral:1,0.05,3") == ("bilateral", {"distance_sigma": 1.0, "range_sigma": 0.05, "radius": 3, "factor": -0.5})
    assert parse_filter("bilateral:5, 2, 10, -0.25") == ("bilateral", {"distance_sigma": 5.0, "range_sigma": 2.0, "radius": 10, "factor": -0.25})
    parsed = parse_filter("gaussian:2")
    assert parse_filter(parsed) is parsed                         # an already parsed spec passes through
    for bad in ("", "gaussian", "gaussian:", "gaussian:x", "gaussian:1,2", "gaussian:0", "gaussian:-1", "gaussian:nan", "gaussian:9",
                "bilateral:1,1", "bilateral:1,1,2.5", "bilateral:1,1,33", "bilateral:1,1,-1", "bilateral:0,1,5", "bilateral:1,0,5",
                "bilateral:1,inf,5", "bilateral:1,1,5,nan", "bilateral:1,1,5,-0.5,7", "median:3", None, 3, ("gaussian", 1)):
        with pytest.raises(ValueError):
            parse_filter(bad)


def test_ply_reader_binary_and_ascii(tmp_path):
    from ply_cases import write_ply
    from speech_anime.datasets.dgrad import read_ply
    rs = np.random.RandomState(0)
    V = rs.normal(0, 1, (11, 3)).astype(np.float32)
    F = rs.randint(0, 11, (7, 3)).astype(np.uint32)
    write_ply(tmp_path / "a.ply", V, F)                              # float x y z, list uchar int: the reference's templates
    v, f = read_ply(str(tmp_path / "a.ply"))
    assert v.dtype == np.float32 and f.dtype == np.uint32 and np.array_equal(v, V) and np.array_equal(f, F)
    # binary with further scalar vertex properties (skipped) and a comment
    rec = np.empty(len(V), np.dtype([("x", "<f4"), ("q", "u1"), ("y", "<f4"), ("z", "<f4"), ("w", "<f8")]))
    rec["x"], rec["y"], rec["z"], rec["q"], rec["w"] = V[:, 0], V[:, 1], V[:, 2], 7, 0.5
    fr = np.empty(len(F), np.dtype([("n", "u1"), ("v", "<u4", (3,))]))
    fr["n"], fr["v"] = 3, F
    head = (f"ply\nformat binary_little_endian 1.0\ncomment made by a test\nelement vertex {len(V)}\nproperty float x\nproperty uchar q\n"
            f"property float y\nproperty float z\nproperty double w\nelement face {len(F)}\nproperty list uchar uint vertex_indices\nend_header\n")
    (tmp_path / "b.ply").write_bytes(head.encode() + rec.tobytes() + fr.tobytes())
    v, f = read_ply(str(tmp_path / "b.ply"))
    assert np.array_equal(v, V) and np.array_equal(f, F)
    # ascii
    text = (f"ply\nformat ascii 1.0\nelement vertex {len(V)}\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n"
            f"element face {len(F)}\nproperty list uchar int vertex_indices\nend_header\n")
    text += "".join(f"{a!r} {b!r} {c!r} 0.25\n" for a, b, c in V.astype(np.float64).tolist())
    text += "".join(f"3 {a} {b} {c}\n" for a, b, c in F.tolist())
    (tmp_path / "c.ply").write_text(text)
    v, f = read_ply(str(tmp_path / "c.ply"))
    assert np.array_equal(v, V) and np.array_equal(f, F)
    # refusals, each with a message
    (tmp_path / "d.ply").write_bytes(head.replace("binary_little_endian", "binary_big_endian").encode() + rec.tobytes() + fr.tobytes())
    (tmp_path / "e.ply").write_text(text.replace(f"3 {F[0, 0]} {F[0, 1]} {F[0, 2]}\n", f"4 {F[0, 0]} {F[0, 1]} {F[0, 2]} 1\n", 1))
    (tmp_path / "f.ply").write_text("not a ply\n")
    (tmp_path / "g.ply").write_text(text.replace("property float y\n", ""))
    (tmp_path / "h.ply").write_bytes((head.encode() + rec.tobytes() + fr.tobytes())[:-5])
    for name, word in (("d", "format"), ("e", "triangle"), ("f", "not a PLY"), ("g", "x, y, z"), ("h", "short")):
        with pytest.raises(ValueError, match=word):
            read_ply(str(tmp_path / f"{name}.ply"))


def test_tfilter_abi_is_bound_and_exported():
    from sdfa_amd import _lib, tfilter
    with open(os.path.join(ROOT, "include", "sdfa_tfilter.h")) as fp:
        hdr = fp.read()
    assert _lib.lib.sdfa_tfilter_abi_version() == tfilter.ABI_VERSION == int(re.search(r"#define SDFA_TFILTER_ABI_VERSION\s+(\d+)", hdr).group(1))
    declared = set(re.findall(r"\b(sdfa_t\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(tfilter.SYMBOLS)
    for name in declared:
        assert hasattr(_lib.lib, name), name
    for macro, value in (("MAX_RADIUS", tfilter.MAX_RADIUS), ("WINDOW_RADIUS", tfilter.WINDOW_RADIUS), ("COLS", tfilter.COLS),
                         ("RUN", tfilter.RUN), ("CLIPS", tfilter.CLIPS), ("GENERIC", tfilter.FLAG_GENERIC)):
        assert int(re.search(rf"#define SDFA_TFILTER_{macro}\s+(\d+)", hdr).group(1)) == value, macro
    assert _lib.lib.sdfa_abi_version() == 5                          # the main header's version is untouched


ROWS, OUT = 1 << 20, 1 << 24          # never dereferenced: every call below is refused on the host
TAPS4 = R.gaussian_taps_ref(1)
REFUSALS = {
    "asymmetric taps": dict(taps=np.r_[TAPS4[:8], np.nextafter(TAPS4[8], 1)]),
    "radius 33": dict(radius=33, taps=np.ones(67) / 67),
    "radius -1": dict(radius=-1),
    "overlap": dict(out=ROWS + 4 * (10 * 45 - 1)),
    "out is rows": dict(out=ROWS),
    "offsets start at 1": dict(off=[1, 10]),
    "offsets end early": dict(off=[0, 4, 9]),
    "offsets run past F": dict(off=[0, 12, 10]),
    "empty clip": dict(off=[0, 4, 4, 10]),
    "no clips": dict(off=[0, 10], n_clips=0),
    "unknown flag bit 1": dict(flags=2),
    "unknown flag bits": dict(flags=1 | 8),
    "no frames": dict(F=0, off=None),
    "no columns": dict(W=0),
    "null rows": dict(rows=None),
    "null out": dict(out=None),
}


def _call(lib, kind, a):
    a = dict(dict(rows=ROWS, out=OUT, F=10, W=45, off=[0, 10], radius=4, taps=TAPS4, flags=0, ds=1.0, rs=1.0, factor=-0.5), **a)
    off = None if a["off"] is None else np.asarray(a["off"], np.int64)
    n_clips = a.get("n_clips", 0 if off is None else len(off) - 1)
    taps = None if a["taps"] is None else np.ascontiguousarray(a["taps"], np.float64)
    optr = None if off is None else off.ctypes.data
    if kind == "fir":
        return lib.sdfa_track_fir(a["rows"], a["out"], a["F"], a["W"], optr, n_clips, None if taps is None else taps.ctypes.data, a["radius"], a["flags"], None)
    return lib.sdfa_track_bilateral(a["rows"], a["out"], a["F"], a["W"], optr, n_clips, a["factor"], a["ds"], a["rs"], a["radius"], None, a["flags"], None)


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_are_made_on_the_host(name):
    from sdfa_amd import _lib, tfilter  # noqa: F401
    a = REFUSALS[name]
    assert _call(_lib.lib, "fir", a) == _lib.EINVAL, name
    assert _lib.lib.sdfa_last_error().decode().startswith("track_fir:")
    if "taps" not in name:
        assert _call(_lib.lib, "bilateral", a) == _lib.EINVAL, name
        assert _lib.lib.sdfa_last_error().decode().startswith("track_bilateral:")


def test_fir_and_bilateral_refuse_their_own_arguments():
    from sdfa_amd import _lib, tfilter  # noqa: F401
    lib = _lib.lib
    assert _call(lib, "fir", dict(taps=None)) == _lib.EINVAL
    for bad in (dict(ds=0.0), dict(ds=-1.0), dict(ds=float("nan")), dict(ds=float("inf")), dict(rs=0.0), dict(rs=-2.0), dict(rs=float("nan")),
                dict(rs=float("inf")), dict(factor=float("nan"))):
        assert _call(lib, "bilateral", bad) == _lib.EINVAL, bad
        assert lib.sdfa_last_error().decode().startswith("track_bilateral:")


def test_binding_checks_arguments_without_a_device():
    import torch
    from sdfa_amd import tfilter
    x = torch.zeros(4, 3)
    for call in (lambda: tfilter.gaussian_filter1d(x, 1.0), lambda: tfilter.bilateral(x), lambda: tfilter.correlate_symmetric(x, [1.0])):
        with pytest.raises(TypeError, match="cuda"):
            call()
    with pytest.raises(ValueError, match="symmetric"):
        tfilter.correlate_symmetric(x, [0.25, 0.5, 0.26])
    with pytest.raises(ValueError, match="odd"):
        tfilter.correlate_symmetric(x, [0.5, 0.5])
    with pytest.raises(ValueError):
        tfilter.bilateral(x, range_sigma=0.0)
    with pytest.raises(ValueError):
        tfilter.bilateral(x, radius=33)
    import math
    assert tfilter.distance_weights(2.0, 2).tolist() == [math.exp(-0.5), math.exp(0.25 * -0.5), 1.0, math.exp(0.25 * -0.5), math.exp(-0.5)]
