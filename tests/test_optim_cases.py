"""Host checks of tests/optim_cases.py (the tables and float64 restatements that tests/test_optim_gpu.py holds the
optimiser kernels against) and of the two entry points' host-side argument checks.  No GPU."""
import numpy as np
import pytest
import torch

import optim_cases as C

ALL_TABLES = dict(C.TABLES, THRESHOLD=C.THRESHOLD)


# ================================================================================================ table invariants

@pytest.mark.parametrize("name", sorted(ALL_TABLES))
def test_table_is_ascending_disjoint_and_inside_its_buffer(name):
    t = ALL_TABLES[name]
    assert t.chunk_seg.dtype == np.int32 and t.chunk_begin.dtype == np.int64 and t.chunk_len.dtype == np.int32
    assert len(t.chunk_seg) == len(t.chunk_begin) == len(t.chunk_len) >= 1
    assert (np.diff(t.chunk_seg) >= 0).all(), "ids must ascend"
    assert t.chunk_seg.min() >= 0 and t.chunk_seg.max() < t.n_segments
    assert (t.chunk_len >= 0).all() and (t.chunk_begin >= 0).all()
    assert (t.chunk_begin + t.chunk_len).max() < t.size, "a tail of untouched floats follows the last chunk"
    assert t.chunk_begin.min() > 0, "untouched floats in front of the first chunk"
    idx, _ = C.elements(t)
    assert idx.size == int(t.chunk_len.sum()) == np.unique(idx).size, "chunks overlap"
    assert t.size <= 210000  # the largest buffer of the GPU tests stays small
    assert not C.covered(t).all()


def test_alignment_table_has_every_length_in_every_class_with_small_gaps():
    t = C.ALIGNMENT
    assert t.n_segments == len(t.chunk_seg) == 4 * len(C.ALIGNMENT_LENGTHS) == 56
    assert C.ALIGNMENT_LENGTHS == [0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 1027]
    seen = {(int(b) % 4, int(n)) for b, n in zip(t.chunk_begin, t.chunk_len)}
    assert seen == {(mod, n) for mod in range(4) for n in C.ALIGNMENT_LENGTHS}
    for s, (mod, n) in C.ALIGNMENT_CLASS.items():
        assert int(t.chunk_seg[s]) == s and int(t.chunk_begin[s]) % 4 == mod and int(t.chunk_len[s]) == n
    gaps = t.chunk_begin[1:] - (t.chunk_begin[:-1] + t.chunk_len[:-1])
    assert gaps.min() >= 1 and gaps.max() <= 5 and len(set(gaps.tolist())) == 5
    assert C.alignment_segment(0, 1027) != C.alignment_segment(1, 1027)


def test_many_chunks_table_has_the_counts_and_mixed_alignments():
    t = C.MANY_CHUNKS
    counts = C.chunks_per_segment(t)
    assert counts.tolist() == C.MANY_COUNTS == [63, 1, 64, 1, 65, 1, 128, 1, 129, 1, 200]
    assert (counts >= 65).sum() == 4 and (counts >= 129).sum() == 2 and counts[C.MANY_SEG_129] == 129
    # every many-chunk segment has a one-chunk neighbour on each side it has a neighbour at all
    for s, k in enumerate(counts):
        if k > 1:
            assert all(counts[j] == 1 for j in (s - 1, s + 1) if 0 <= j < len(counts))
    assert set(t.chunk_len.tolist()) == set(range(1, 10))
    assert t.chunk_len.tolist()[:18] == list(range(1, 10)) * 2
    for s, k in enumerate(counts):
        if k >= 63:  # both branches of seg_sumsq_kernel feed each long sum
            assert {int(b) % 4 for b in t.chunk_begin[t.chunk_seg == s]} == {0, 1, 2, 3}
    # the chunks the wrong-scale detector plants in: first, 65th and last of the 129
    assert (t.chunk_seg == C.MANY_SEG_129).sum() == 129


def test_empty_segment_tables():
    for name, ids in C.EMPTY_IDS.items():
        t = C.TABLES[name]
        counts = C.chunks_per_segment(t)
        assert [s for s in range(t.n_segments) if counts[s] == 0] == ids, name
    t = C.EMPTY_MIDDLE
    assert sorted(set(t.chunk_seg.tolist())) == [0, 1, 3, 4, 7] and t.n_segments == 10
    assert 0 in t.chunk_len.tolist()  # a zero-length chunk inside a used segment
    assert int(C.EMPTY_FRONT.chunk_seg[0]) == 2
    assert len(C.ONE_CHUNK.chunk_seg) == 1 and C.ONE_CHUNK.n_segments == 3


def test_long_table_and_full_chunks():
    t = C.LONG_TABLE
    counts = C.chunks_per_segment(t)
    assert len(t.chunk_seg) == 70000 and t.n_segments == 2001
    assert counts[C.LONG_SEG] == 40000 == 625 * 64 and (np.delete(counts, C.LONG_SEG) == 15).all()
    assert set(t.chunk_len.tolist()) == {1, 2, 3}
    assert {int(b) % 4 for b in t.chunk_begin[t.chunk_seg == C.LONG_SEG]} == {0, 1, 2, 3}
    f = C.FULL_CHUNKS
    assert f.chunk_len.tolist() == [16384, 16384, 16384, 5] and f.n_segments == 1
    assert (f.chunk_begin % 64 == 0).all()  # 256-byte aligned, as the trainer's flat buffer
    assert (f.chunk_begin[1:] == f.chunk_begin[:-1] + f.chunk_len[:-1]).all()


@pytest.mark.parametrize("name", sorted(C.TABLES))
def test_exact_gradients_keep_every_segment_below_2_to_24(name):
    """The exactness condition: integers times 2^-6 whose squares sum, per segment, to an integer below 2^24 -- then
    the float64 sumsq is representable in fp32 and is what any fp32 summation order gives."""
    t = C.TABLES[name]
    g, sumsq, clipped = C.exact_case(name)
    total = C.check_exact(g, t)
    assert total.max() < 2 ** 24
    assert np.array_equal(sumsq, total * 2.0 ** -12)
    assert np.array_equal(sumsq.astype(np.float32).astype(np.float64), sumsq)
    assert (g[~C.covered(t)] == C.GAP_FILL).all()
    norm = np.sqrt(sumsq)
    # sumsq is a multiple of 2^-12 and clip^2 = 2^-2 is one too: a segment is either exactly on the threshold (sqrtf is
    # exact there) or 2^-10 of clip^2 away from it, 2^14 ulps -- the fp32 norm cannot decide otherwise than float64's
    assert C.EXACT_CLIP ** 2 == 0.25
    assert ((sumsq == 0.25) | (np.abs(sumsq / 0.25 - 1) >= 2.0 ** -10)).all()
    if name in ("ALIGNMENT", "MANY_CHUNKS", "EMPTY_MIDDLE", "EMPTY_FRONT", "LONG_TABLE"):
        assert (norm > C.EXACT_CLIP).any() and (norm[C.chunks_per_segment(t) > 0] <= C.EXACT_CLIP).any()
    if name == "FULL_CHUNKS":
        assert norm[0] > C.EXACT_CLIP
    # the narrowing rule itself, on a segment long enough to need it
    long_seg = C.make_table([(0, 1, 2 ** 18)])
    narrow = C.exact_grad(np.random.default_rng(0), long_seg)
    assert set(np.unique(narrow[1:1 + 2 ** 18] / C.GRAD_UNIT).tolist()) == {-1.0, 0.0, 1.0}
    C.check_exact(narrow, long_seg)


def test_threshold_patterns_sit_exactly_on_and_just_past_the_clip():
    for unit in (1.0, C.GRAD_UNIT):
        g = C.threshold_grad(unit)
        sumsq, clipped = C.clip_ref(g, C.THRESHOLD, C.THRESHOLD_CLIP * unit)
        assert (sumsq / unit ** 2).tolist() == [25.0, 25.0, 0.0, 26.0, 25.0, 26.0]
        assert np.float32(np.sqrt(np.float32(25.0 * unit ** 2))) == np.float32(5.0 * unit)
        idx, seg = C.elements(C.THRESHOLD)
        moved = np.isin(seg, C.THRESHOLD_SCALED)
        assert np.array_equal(clipped[idx][~moved], g[idx][~moved].astype(np.float64))
        want = g[idx][moved].astype(np.float64) * 5.0 / np.sqrt(26.0)
        np.testing.assert_allclose(clipped[idx][moved], want, rtol=1e-15)


def test_real_gradients_stay_clear_of_the_clip():
    for name in C.REAL_TABLES:
        t = C.TABLES[name]
        g, draws = C.real_grad(7, name)
        norm = np.sqrt(C.clip_ref(g, t, C.REAL_CLIP[name])[0])
        assert (np.abs(norm / C.REAL_CLIP[name] - 1) > C.REAL_MARGIN).all() and 1 <= draws <= 8
        assert np.isnan(g[~C.covered(t)]).all() and np.isfinite(g[C.covered(t)]).all()
        assert (norm > C.REAL_CLIP[name]).any()
        if t.n_segments > 1:
            assert (norm <= C.REAL_CLIP[name]).any()


def test_sumsq_depth_reads_the_kernels_chains():
    # one float4 trip per thread, no tail, one chunk: 1 + 4 + 6 + 3 + 1 + 6
    assert C.sumsq_depth(1024, 1, True) == 21
    assert C.sumsq_depth(1027, 1, True) == 22 and C.sumsq_depth(1027, 1, False) == 1 + 5 + 9 + 7
    assert C.sumsq_depth(16384, 4, True) == 1 + 64 + 9 + 7
    assert C.sumsq_depth(3, 40000, False) == 1 + 1 + 9 + 625 + 6
    assert C.sumsq_depth(0, 1, True) == 17
    b = C.sumsq_bound(C.FULL_CHUNKS)
    assert b.shape == (1,) and b[0] == 82 * C.U
    assert (C.sumsq_bound(C.EMPTY_MIDDLE)[C.EMPTY_MIDDLE_IDS] == 0).all()


# ================================================================================================ restatements

def _per_tensor(table):
    """The segments as lists of flat indices (an independent walk over the table)."""
    out = [[] for _ in range(table.n_segments)]
    for s, b, n in zip(table.chunk_seg.tolist(), table.chunk_begin.tolist(), table.chunk_len.tolist()):
        out[s].extend(range(b, b + n))
    return out


@pytest.mark.parametrize("name", ["ALIGNMENT", "MANY_CHUNKS", "EMPTY_MIDDLE", "EMPTY_FRONT", "ONE_CHUNK", "FULL_CHUNKS"])
def test_clip_ref_is_g_clip_over_max_norm_clip_per_tensor(name):
    t = C.TABLES[name]
    rng = np.random.default_rng(3)
    g = rng.standard_normal(t.size) * 0.05
    clip = 0.4
    sumsq, clipped = C.clip_ref(g, t, clip)
    gt = torch.from_numpy(g)
    want = gt.clone()
    for s, ids in enumerate(_per_tensor(t)):
        x = gt[ids]
        norm = torch.linalg.vector_norm(x)
        assert abs(float(norm) ** 2 - sumsq[s]) <= 1e-12 * max(sumsq[s], 1e-30)
        want[ids] = x * clip / torch.clamp(norm, min=clip)
    np.testing.assert_allclose(clipped, want.numpy(), rtol=1e-14, atol=0)
    gaps = ~C.covered(t)
    assert np.array_equal(clipped[gaps], g[gaps])
    assert (sumsq[C.chunks_per_segment(t) == 0] == 0).all()


def test_clip_ref_nonfinite_rules():
    t = C.MANY_CHUNKS
    g = C.exact_case("MANY_CHUNKS")[0].copy()
    idx, seg = C.elements(t)
    nan_at, inf_at = idx[seg == 4][100], idx[seg == 6][7]
    g[nan_at], g[inf_at] = np.nan, np.inf
    sumsq, clipped = C.clip_ref(g, t, C.EXACT_CLIP)
    assert np.isnan(sumsq[4]) and np.isinf(sumsq[6]) and np.isfinite(np.delete(sumsq, [4, 6])).all()
    keep = idx[seg == 4]
    assert np.array_equal(clipped[keep], g[keep].astype(np.float64), equal_nan=True)  # NaN norm: as it is
    zeroed = idx[(seg == 6) & (idx != inf_at)]
    assert (clipped[zeroed] == 0).all() and np.array_equal(np.signbit(clipped[zeroed]), np.signbit(g[zeroed]))
    assert np.isnan(clipped[inf_at])


def test_fused_ref_matches_torch_adam_and_lerp_over_three_steps():
    """eps = 0 (torch's and TensorFlow's placements of epsilon coincide), non-zero gradients, hyper-parameters that
    float32 holds exactly: clip_adam_ema_ref == per-tensor g clip / max(norm, clip) -> torch.optim.Adam -> torch.lerp in
    float64."""
    t = C.MANY_CHUNKS
    lr0, b1, b2, decay, clip = 2.0 ** -7, 0.875, 1 - 2.0 ** -10, 0.75, 0.4
    rng = np.random.default_rng(5)
    tensors = _per_tensor(t)
    p0 = rng.standard_normal(t.size)
    params = [torch.nn.Parameter(torch.from_numpy(p0[ids])) for ids in tensors]
    opt = torch.optim.Adam(params, lr=lr0, betas=(b1, b2), eps=0.0)
    shadows = [q.detach().clone() for q in params]
    ref = [p0.copy(), np.zeros(t.size), np.zeros(t.size), p0.copy()]
    n_scaled = 0
    for step in range(1, 4):
        lr = lr0 / step  # (a schedule: 2^-7, 2^-8, 2^-7 / 3 rounded to float32 on both sides)
        lr = float(np.float32(lr))
        g = rng.standard_normal(t.size) * 0.05
        g[g == 0] = 0.05
        for group in opt.param_groups:
            group["lr"] = lr
        for q, ids in zip(params, tensors):
            x = torch.from_numpy(g[ids])
            norm = torch.linalg.vector_norm(x)
            n_scaled += int(norm > clip)
            q.grad = x * clip / torch.clamp(norm, min=clip)
        opt.step()
        for sh, q in zip(shadows, params):
            sh.copy_(torch.lerp(sh, q.detach(), 1 - decay))
        *ref, sumsq = C.clip_adam_ema_ref(ref[0], ref[1], ref[2], ref[3], g, t, clip, lr, b1, b2, 0.0, step, decay)
        assert C.adam_lr_t(lr, b1, b2, step) == lr * np.sqrt(1 - b2 ** step) / (1 - b1 ** step)
        for q, sh, ids in zip(params, shadows, tensors):
            np.testing.assert_allclose(ref[0][ids], q.detach().numpy(), rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(ref[3][ids], sh.numpy(), rtol=1e-12, atol=1e-14)
    assert 0 < n_scaled < 3 * len(tensors)
    gaps = ~C.covered(t)
    assert np.array_equal(ref[0][gaps], p0[gaps]) and not ref[1][gaps].any() and not ref[2][gaps].any()
    # without clipping the restatement is adam_ref with scale 1, and reports no norms
    out = C.clip_adam_ema_ref(p0, np.zeros(t.size), np.zeros(t.size), None, g, t, 0.0, lr0, b1, b2, 1e-8, 1, decay)
    assert out[3] is None and out[4] is None
    idx, _ = C.elements(t)
    want = C.adam_ref(p0[idx], np.zeros(idx.size), np.zeros(idx.size), g[idx], lr0, b1, b2, 1e-8, 1, 1.0)
    assert np.array_equal(out[0][idx], want[0]) and np.array_equal(out[2][idx], want[2])


# ================================================================================================ argument checks

FAKE = 4096  # a non-NULL pointer that is never dereferenced: every status below comes back before a launch


def _clip(lib, n_chunks=3, n_segments=2, clip=1.0, floats=5, grads=FAKE, seg=FAKE, begin=FAKE, length=FAKE, sumsq=FAKE):
    return lib.mpsr_clip_by_norm_segments(grads, seg, begin, length, n_chunks, sumsq, floats, n_segments, clip, None)


def _fused(lib, n_chunks=3, n_segments=2, clip=1.0, floats=5, step=1, p=FAKE, g=FAKE, m=FAKE, v=FAKE, shadow=FAKE,
           seg=FAKE, begin=FAKE, length=FAKE, sumsq=FAKE):
    return lib.mpsr_clip_adam_ema_step(p, g, m, v, shadow, seg, begin, length, n_chunks, sumsq, floats, n_segments, clip,
                                       1e-3, 0.9, 0.999, 1e-8, step, 0.99, None)


def test_optimiser_entry_points_check_their_arguments_on_the_host():
    """Statuses come back before anything touches the device (status 1 / 3 + message); no pointer is dereferenced."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    INVALID, WORKSPACE = 1, 3
    assert _clip(lib, n_chunks=-1) == INVALID and b"bad arguments" in lib.mpsr_last_error()
    assert _clip(lib, n_segments=-1) == INVALID
    assert _clip(lib, clip=0.0) == INVALID and _clip(lib, clip=-1.0) == INVALID
    assert _clip(lib, clip=float("nan")) == INVALID
    for name in ("grads", "seg", "begin", "length", "sumsq"):
        assert _clip(lib, **{name: None}) == INVALID and b"null" in lib.mpsr_last_error(), name
    assert _clip(lib, floats=4) == WORKSPACE and b"n_segments + n_chunks" in lib.mpsr_last_error()
    assert b"clip_by_norm_segments" in lib.mpsr_last_error()
    assert _clip(lib, floats=0) == WORKSPACE
    assert lib.mpsr_clip_by_norm_segments(None, None, None, None, 0, None, 0, 0, 1.0, None) == 0
    assert lib.mpsr_clip_by_norm_segments(None, None, None, None, 0, None, 0, 4, 1.0, None) == 0

    assert _fused(lib, n_chunks=-1) == INVALID and b"bad arguments" in lib.mpsr_last_error()
    assert _fused(lib, n_segments=-1) == INVALID
    assert _fused(lib, step=0) == INVALID and _fused(lib, step=-3) == INVALID
    for name in ("p", "g", "m", "v", "seg", "begin", "length"):
        assert _fused(lib, **{name: None}) == INVALID and b"null" in lib.mpsr_last_error(), name
    assert _fused(lib, sumsq=None) == INVALID and b"sumsq" in lib.mpsr_last_error()
    assert _fused(lib, n_segments=0) == INVALID and b"sumsq" in lib.mpsr_last_error()
    assert _fused(lib, floats=4) == WORKSPACE and b"n_segments + n_chunks" in lib.mpsr_last_error()
    assert b"clip_adam_ema_step" in lib.mpsr_last_error()
    assert lib.mpsr_clip_adam_ema_step(None, None, None, None, None, None, None, None, 0, None, 0, 0, 1.0, 1e-3, 0.9,
                                       0.999, 1e-8, 1, 0.99, None) == 0
    assert lib.mpsr_clip_adam_ema_step(None, None, None, None, None, None, None, None, 0, None, 0, 0, 0.0, 1e-3, 0.9,
                                       0.999, 1e-8, 1, 0.99, None) == 0
