"""CPU: the exact-operand method of tests/gemm_ref.py detects the faults it is meant for, and its conditions hold.

  * every case of every table is inside the bit budget (so the GPU comparison may be an equality of words);
  * a numpy emulation of a tiled GEMM — K-tiles of 64, fp32 accumulation in a shuffled order, three, two or one terms,
    planes read at their offsets — equals the reference bit for bit on every host-sized case;
  * each mutant of that emulation (gemm_ref.MUTANTS) differs from the reference on at least one listed case;
  * the split-output reference is the two-rounding split the older GEMM tests use (_split_planes);
  * the shape lists cover every (M, N), (M, K), (N, K) pair of the edge values for
    every dtype, both tile widths and both K loops of the 128-tile kernel, and the route of every persistent case.
"""
import numpy as np
import pytest
import torch

import gemm_ref as R

HOST_WORK = 3_000_000          # M * N * K of the cases the emulation runs on
DEV = torch.device("cpu")


def _host_cases():
    seen, out = set(), []
    for c in R.ALL_EXACT_CASES:
        if c.M * c.N * c.K <= HOST_WORK and max(c.a_gap, c.c_gap) < R.FAR and c.id not in seen:
            seen.add(c.id)
            out.append(c)
    return out


HOST_CASES = _host_cases()


def _reference(c):
    o = R.operands(c, DEV)
    bias, res = R.epilogue_operands(c, DEV)
    acc = R.products(o, c.terms, c.split)
    assert np.array_equal(R.products_int64(o, c.terms, c.split), acc.numpy() * 64), c.id      # float64 product == int64 product
    want = R.expected(c, acc, bias, res)
    return o, bias, res, {k: v.float().numpy() for k, v in want.items()}


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def test_every_case_is_inside_the_bit_budget():
    assert len(R.ALL_EXACT_CASES) > 1000
    for c in R.ALL_EXACT_CASES:
        assert R.in_budget(c), c.id
    # the condition bites: the same ranges at a K that is too long, or a bias that leaves the fp16 range, are refused
    assert not R.in_budget(R.make_case("fp16x3", 128, 128, 16384, R.EPI_BIAS_F32, terms=3))
    assert not R.in_budget(R.make_case("fp16", 128, 128, 4096, R.EPI_BIAS_16))
    assert R.in_budget(R.make_case("fp16", 128, 128, 4096, R.EPI_BIAS_16, amax=2))
    assert R.in_budget(R.make_case("fp16x3", 128, 128, 4096, R.EPI_BIAS_F32, terms=3))       # 16.5 * 4096 * 64 < 2^23
    assert not R.in_budget(R.make_case("fp16x3", 128, 128, 1024, R.EPI_BIAS_F32, terms=3, oscale=2.0 ** -12, bias_max=3000))


def test_shape_lists_cover_every_pair_tile_width_and_loop():
    for dt in R.DTYPES:
        shapes = R.edge_shapes(dt)
        ks = R.EDGE_K_F32 if dt == "fp32" else R.EDGE_K
        assert 40 <= len(shapes) <= 90
        for m in R.EDGE_M:
            for n in R.EDGE_N:
                assert any(s[0] == m and s[1] == n for s in shapes), (dt, m, n)
            for k in ks:
                assert any(s[0] == m and s[2] == k for s in shapes), (dt, m, k)
        for n in R.EDGE_N:
            for k in ks:
                assert any(s[1] == n and s[2] == k for s in shapes), (dt, n, k)
        if dt != "fp32":
            variants = {R.tile128_variant(*s) + (s[1] >= 64,) for s in shapes}
            for bn in (64, 128):
                for loop in ("dma", "plain"):
                    assert (bn, loop, True) in variants, (dt, bn, loop)         # with N >= 64: whole and ragged column tiles
            assert (128, "dma", False) in variants and (128, "plain", False) in variants
        runs = R.EDGE_CASES[dt]
        assert {c.epi for c in runs} == {0, 2, 3}
        assert {c.terms for c in runs} == ({3, 2, 1} if dt == "fp16x3" else {3, 1} if dt == "bf16x3" else {1})
        if dt in R.SPLIT:
            assert {c.oscale for c in runs} == {1.0, 2.0 ** -12} and all(c.force == "128" for c in runs)
        assert all(c.expected_route in ("128", "f32") for c in runs)


def test_persistent_cases_reach_the_routes_they_are_listed_for():
    by = {}
    for c in R.PERSISTENT_CASES:
        by.setdefault(c.expected_route, []).append(c)
    assert set(by) == {"g256", "x3", "x3+128", "gres"}
    assert {(c.M, c.N) for c in by["g256"] if c.dtype in R.PLAIN16} == set(R.G256_SHAPES)
    assert {c.K for c in by["g256"]} == set(R.PERSISTENT_K)
    assert {c.dtype for c in by["g256"]} == set(R.PLAIN16) | set(R.SPLIT)        # split: one term (gemm256_kernel<SPLIT>)
    assert {(c.M, c.N) for c in by["x3"]} == set(R.X3_SHAPES) | {R.X3_TWO_ROUNDS}
    assert {(c.dtype, c.terms) for c in by["x3"]} == {("fp16x3", 3), ("bf16x3", 3), ("fp16x3", 2)}
    assert {c.epi for c in by["x3"]} == {0, 2, 3} and {c.K for c in by["x3"]} == set(R.PERSISTENT_K)
    assert {(c.M, c.N) for c in by["x3+128"]} == {R.X3_SEAM}
    assert R.x3_main_rows("fp16x3", 0, *R.X3_SEAM, 192, 3) == 4096                  # the seam: 256 tiles, then 1024 rows
    tiles = sorted({(c.M // 256) * (c.N // 128) for c in by["gres"]})
    W = R.GRES_W
    assert tiles == [1, W - 1, W, W + 1, 2 * W + 3]
    for c in by["gres"]:
        assert R.gemm_res_supports(c.dtype, c.epi, c.M, c.N, c.K), c.id
        assert (c.K // 64) * c.terms >= 2, c.id                                    # launch_gemm_res: two ring entries at least
    assert {(c.dtype, c.terms, min(x.K for x in by["gres"] if (x.dtype, x.terms) == (c.dtype, c.terms))) for c in by["gres"]} == \
        {("bf16", 1, 128), ("fp16", 1, 128), ("fp16x3", 3, 64), ("bf16x3", 3, 64), ("fp16x3", 1, 128)}
    # 208 tiles is a round that is taken although it is not full; 204 would leave the rows to the 128-tile kernel
    assert R.route("fp16x3", 0, 3328, 4096, 128, 3) == "x3" and R.route("fp16x3", 0, 204 * 256, 256, 128, 3) == "128"
    assert R.route("bf16x3", 0, 3328, 4096, 128, 2) == "128" and R.route("fp32", 0, 4096, 4096, 128) == "f32"


def test_emulation_equals_the_reference_on_every_host_case():
    assert len(HOST_CASES) > 500
    rng = np.random.default_rng(5)
    for c in HOST_CASES:
        o, bias, res, want = _reference(c)
        got = R.emulate(c, o, bias, res, rng)
        assert set(got) == set(want), c.id
        assert _same(got, want), c.id


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_detected(mutant):
    rng = np.random.default_rng(11)
    caught, ran = [], 0
    for c in HOST_CASES[::7] + [c for c in R.OFFSET_CASES if c.M * c.N * c.K <= HOST_WORK and c.a_gap < R.FAR]:
        o, bias, res, want = _reference(c)
        ran += 1
        if not _same(R.emulate(c, o, bias, res, rng, mutant=mutant), want):
            caught.append(c.id)
    print(f"mutant {mutant}: detected on {len(caught)} of {ran} cases")
    assert caught, mutant


def test_split_reference_is_the_two_rounding_split_of_the_older_tests():
    from test_gpu_parity import _split_planes
    for c in (R.make_case("fp16x3", 129, 136, 72, 0, terms=3), R.make_case("bf16x3", 65, 200, 128, 0, terms=3),
              R.make_case("fp16x3", 63, 72, 320, 0, terms=2, oscale=2.0 ** -12)):
        o = R.operands(c, DEV)
        bias, res = R.epilogue_operands(c, DEV)
        acc = R.products(o, c.terms, True)
        v32 = R.value(c, acc, bias, res)
        want = R.expected(c, acc, bias, res)
        td = R.OPERAND_T[c.dtype]
        old = _split_planes(v32, td)
        assert torch.equal(R.words(old[0]), R.words(want["hi"])) and torch.equal(R.words(old[1]), R.words(want["lo"]))
        # and the independent bit arithmetic of the emulation agrees with torch's conversions, ties included
        hi = R.round16_np(v32.numpy(), td)
        assert np.array_equal(hi, want["hi"].float().numpy())
        assert np.array_equal(R.round16_np(v32.numpy() - hi, td), want["lo"].float().numpy())
        if c.oscale == 1.0:
            ulp = 2.0              # of both formats in the range looked at: fp16 in [2048, 4096), bf16 in [256, 512)
            lim = 2048 if td == torch.float16 else 256
            big = v32[(v32.abs() > lim) & (v32.abs() < 2 * lim)]
            assert bool(((big % ulp) != 0).any()), "the integers must hit ties of the 16-bit store"


def test_guarded_views_catch_a_stray_write_and_a_stray_read():
    for td in (torch.float32, torch.float16, torch.bfloat16):
        t = R.guarded((5, 8), td, DEV)
        assert t.shape == (5, 8) and t.data_ptr() % 16 == 0 and R.guards_intact(t)
        t.zero_()
        assert R.guards_intact(t)
        flat = torch.empty(0, dtype=td).set_(t.untyped_storage())
        assert bool(torch.isnan(flat[:R.GAP].float()).all()) and bool(torch.isnan(flat[R.GAP + 40:].float()).all())
        flat[R.GAP + 40] = 0
        assert not R.guards_intact(t)
    p = R.Planes((3, 8), torch.float16, DEV, lo_off=24 + 16)
    assert p.intact() and p.lo.data_ptr() - p.hi.data_ptr() == 80
    p.put(torch.ones(3, 8), torch.zeros(3, 8))
    assert p.intact()
    p.raw[p.before + 24] = 0
    assert not p.intact()


def test_fp32_dot_bound_and_gelu_helpers():
    g = torch.Generator().manual_seed(3)
    A, W = torch.randn(37, 48, generator=g), torch.randn(24, 48, generator=g)
    b = torch.randn(24, generator=g)
    exact = A.double() @ W.double().t() + b.double()
    seq = torch.zeros(37, 24)
    for k in range(48):
        seq += A[:, k:k + 1] * W[:, k].unsqueeze(0)
    assert bool(((seq + b).double() - exact).abs().le(R.dot_bound(A, W, b, None)).all())
    x = R.gelu_grid(200, DEV)
    assert x.numel() == 200 and x.min() == -100 and x.max() == 100 and bool((x == 0).sum() == 2)
    assert float(R.half_ulp16(torch.tensor([1.0, 1.5, 2048.0, 1e-9], dtype=torch.float64), torch.float16)[2]) == 1.0
    assert float(R.half_ulp16(torch.tensor([1.0], dtype=torch.float64), torch.bfloat16)[0]) == 2.0 ** -8
    assert abs(float(R.gelu64(torch.tensor([1.0]))[0]) - 0.8413447460685429) < 1e-15
