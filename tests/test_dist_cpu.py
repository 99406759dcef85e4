"""gloo tests of the N>1 path's sharding and chunked all-gather bookkeeping (CPU tensors): world size 2, and -- round 4 -- the
world-size-8 rehearsal of every gather mode (FrameGatherer even / ragged / a rank without frames / ranks with fewer chunks than
the longest shard, ExpandGatherer, run_chunks over two steps), which is what bench.py --gpus 8 runs over RCCL."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


# The workers end with gloo's own host-side barrier: dist.barrier() also opens the GPU runtime in every rank, and eight ranks with
# the GPU open next to the test process exceed what a shared GPU machine allows.


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, n_clips, frames_per_clip, width, chunk, q):
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "sdfa-2019_amd"))
    from sdfa_amd import dist as sd
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = sd.shard_range(n_clips, rank, world)
    # stand-in for the per-frame output: row value encodes (global clip, frame-in-clip, column)
    rows = []
    for c in range(lo, hi):
        for f in range(frames_per_clip[c]):
            rows.append(c * 1000.0 + f + np.arange(width) * 1e-3)
    local = torch.tensor(np.asarray(rows, np.float32).reshape(-1, width))
    counts = sd.frame_counts_all(local.shape[0])
    g = sd.FrameGatherer(counts, width, torch.float32, "cpu", chunk)
    calls = []
    for step in range(2):       # two "steps" of bench.py's loop shape: a rank that skipped a collective would mispair here
        g.buf.zero_()
        sd.run_chunks(local.shape[0], chunk, g, lambda f0, f1: (calls.append((f0, f1)), local[f0:f1])[1])
    assert all(f1 > f0 for f0, f1 in calls)
    out = g.gathered()
    per_rank = torch.cat(g.rows(1), 0)
    assert per_rank.shape[0] == counts[1]
    q.put((rank, counts, out.numpy()))
    dist.monitored_barrier()
    dist.destroy_process_group()


# [9, 3]: rank 0 holds 3 chunks of 4 frames, rank 1 one -- different chunk counts per rank (the bench loop hung there)
@pytest.mark.parametrize("frames_per_clip", [[5, 5, 5, 5], [3, 9, 4, 1, 7], [9, 3], [2, 11]])
def test_sharded_gather_reassembles_clip_order(frames_per_clip):
    world, width, chunk = 2, 6, 4
    n_clips = len(frames_per_clip)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n_clips, frames_per_clip, width, chunk, q)) for r in range(world)]
    for p in procs: p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs: p.join(timeout=60)
    expect = np.asarray([c * 1000.0 + f + np.arange(width) * 1e-3 for c in range(n_clips) for f in range(frames_per_clip[c])], np.float32)
    for rank, counts, out in res:
        assert sum(counts) == len(expect)
        assert np.array_equal(out, expect), rank


class _LinearEngine:
    """Stand-in for Engine on CPU: the expansion is a fixed linear map of the coefficients, as the PCA stage is."""
    coef_dim, out_dim = 5, 12

    def __init__(self):
        rs = np.random.RandomState(3)
        self.basis = torch.tensor(rs.normal(0, 1, (self.coef_dim, self.out_dim)).astype(np.float32))
        self.mean = torch.tensor(rs.normal(0, 1, self.out_dim).astype(np.float32))

    def expand_coef(self, coef, out=None):
        # the same float32 operations for a row whatever rows come with it, like sdfa_expand_coef (a CPU matmul's kernel -- and so
        # its last bit -- can depend on the number of rows and on the host's instruction set)
        r = self.mean.expand(coef.shape[0], self.out_dim)
        for k in range(self.coef_dim):
            r = r + coef[:, k:k + 1] * self.basis[k]
        if out is None:
            return r
        out.copy_(r)
        return out


def _expand_worker(rank, world, port, counts_in, chunk, q):
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "sdfa-2019_amd"))
    from sdfa_amd import dist as sd
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = _LinearEngine()
    n = counts_in[rank]
    coef = torch.tensor(np.random.RandomState(100 + rank).normal(0, 1, (n, eng.coef_dim)).astype(np.float32))
    counts = sd.frame_counts_all(n)
    g = sd.ExpandGatherer(counts, eng, "cpu", chunk)
    for step in range(2):
        g.buf.fill_(float("nan"))

        def compute(f0, f1):
            eng.expand_coef(coef[f0:f1], out=g.own(f0, f1))         # the regressor writes this rank's rows in place
            return coef[f0:f1]
        sd.run_chunks(n, chunk, g, compute)
    q.put((rank, counts, g.gathered().numpy().copy()))
    dist.monitored_barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("counts", [[8, 8], [9, 3], [2, 11]])
def test_expand_gather_rebuilds_every_ranks_rows(counts):
    """ExpandGatherer: coefficients travel, rows are rebuilt on every rank, rank order, even and ragged shards."""
    world, chunk = 2, 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_expand_worker, args=(r, world, port, counts, chunk, q)) for r in range(world)]
    for p in procs: p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs: p.join(timeout=60)
    eng = _LinearEngine()
    expect = np.concatenate([eng.expand_coef(torch.tensor(np.random.RandomState(100 + r).normal(0, 1, (counts[r], 5)).astype(np.float32))).numpy()
                             for r in range(world)])
    for rank, got_counts, out in res:
        assert got_counts == counts
        assert np.array_equal(out, expect), rank


def test_shard_range_partitions():
    import sys
    from sdfa_amd.dist import shard_range
    for n in (0, 1, 7, 32, 256, 257):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


# ---------------------------------------------------------------------------------------------------- world size 8 (and 2)
def _spawn(world, target, args, timeout=240):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (q,)) for r in range(world)]
    for p in procs: p.start()
    try:
        res = [q.get(timeout=timeout) for _ in procs]
    finally:
        for p in procs: p.join(timeout=60)
        for p in procs:
            if p.is_alive():
                p.kill()
    return sorted(res, key=lambda r: r[0])


def _rows_of(rank, n, width):
    """Row f of rank r: r * 1e4 + f in column 0, then a ramp -- any misplaced row is visible."""
    return (rank * 1e4 + np.arange(n, dtype=np.float64)[:, None] + np.arange(width)[None, :] * 1e-2).astype(np.float32)


def _multi_worker(rank, world, port, cases, width, q):
    """Several (counts, chunk) cases through ONE process group: FrameGatherer over two steps, then ExpandGatherer."""
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(here, "sdfa-2019_amd"))
    from sdfa_amd import dist as sd
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    eng = _LinearEngine()
    for counts_in, chunk in cases:
        n = counts_in[rank]
        local = torch.tensor(_rows_of(rank, n, width))
        counts = sd.frame_counts_all(n)
        assert counts == list(counts_in)
        g = sd.FrameGatherer(counts, width, torch.float32, "cpu", chunk)
        assert g.n_chunks == (max(counts) + chunk - 1) // chunk
        n_calls = 0
        for step in range(2):                     # a rank that skipped a collective in step 0 would mispair in step 1
            g.buf.fill_(float("nan"))
            seen = []
            sd.run_chunks(n, chunk, g, lambda f0, f1: (seen.append((f0, f1)), local[f0:f1] + step)[1])
            assert seen == [(f0, min(n, f0 + chunk)) for f0 in range(0, n, chunk)]
            n_calls += len(seen)
        gathered = g.gathered().numpy().copy()
        per_rank = [torch.cat(g.rows(r), 0).numpy().copy() for r in range(world)]
        # the coefficient form on the same shards
        coef = torch.tensor(np.random.RandomState(100 + rank).normal(0, 1, (n, eng.coef_dim)).astype(np.float32))
        x = sd.ExpandGatherer(counts, eng, "cpu", chunk)
        for step in range(2):
            x.buf.fill_(float("nan"))

            def compute(f0, f1):
                eng.expand_coef(coef[f0:f1], out=x.own(f0, f1))
                return coef[f0:f1]
            sd.run_chunks(n, chunk, x, compute)
        out.append((gathered, per_rank, x.gathered().numpy().copy(), n_calls))
    q.put((rank, out))
    dist.monitored_barrier()
    dist.destroy_process_group()


WORLD8_CASES = [
    ([8] * 8, 4),                           # even shards, two chunks each: the bench case (one all_gather_into_tensor per chunk, no staging)
    ([5] * 8, 4),                           # even shards whose last chunk is short
    ([9, 3, 4, 1, 7, 12, 2, 5], 4),         # ragged: 1 .. 3 chunks per rank
    ([6, 0, 6, 6, 0, 6, 6, 6], 4),          # two ranks hold no frames at all (fewer clips than ranks)
    ([1, 1, 1, 1, 1, 1, 1, 17], 4),         # one long shard: seven ranks join four collectives with nothing of their own
    ([3] * 8, 8),                           # a chunk larger than any shard
]


@pytest.mark.parametrize("world", [2, 8])
def test_gather_modes_at_world_size(world):
    """The N = 8 rehearsal VERDICT r3 asked for (SCALE stays unmeasured on hardware; this is the bookkeeping, not the links):
    every rank must end each step holding every rank's rows, in rank order, bit for bit, in the row form (FrameGatherer) and the
    coefficient form (ExpandGatherer), whatever the shard sizes."""
    width = 6
    cases = [(c[:world], ch) for c, ch in WORLD8_CASES]
    res = _spawn(world, _multi_worker, (cases, width))
    assert [r for r, _ in res] == list(range(world))
    eng = _LinearEngine()
    for ci, (counts, chunk) in enumerate(cases):
        expect = np.concatenate([_rows_of(r, counts[r], width) + 1 for r in range(world)])          # step 1's rows (local + 1)
        expect_x = np.concatenate([eng.expand_coef(torch.tensor(np.random.RandomState(100 + r).normal(0, 1, (counts[r], eng.coef_dim)).astype(np.float32)))
                                   .numpy().reshape(counts[r], eng.out_dim) for r in range(world)])
        for rank, out in res:
            gathered, per_rank, expanded, n_calls = out[ci]
            assert np.array_equal(gathered, expect), (world, ci, rank)
            for r in range(world):
                assert np.array_equal(per_rank[r], _rows_of(r, counts[r], width) + 1), (world, ci, rank, r)
            assert np.array_equal(expanded, expect_x), (world, ci, rank)
            assert n_calls == 2 * ((counts[rank] + chunk - 1) // chunk)
