"""CPU: pins tests/critic_restatement.py (the float64 reference of test_gpu_critic_fp64.py) to what the project already trusts
— oracle/nets.critic_value, the reference's golden, float64 autograd — checks the emulation of k_split_w1 (hi + mid + lo == w
exactly, zero padding), and checks that every GPU case is sensitive: each mutation below moves every output that depends on
the mutated input by at least 10x the tolerance the GPU test applies to that output (all of it computable without a GPU).

Which output depends on what. Forward: value, h1 and h2 depend on every count column, byte and clock. Backward: the kernel
takes h1 / h2 as inputs, so the counts reach dW1's count columns only and the clocks dW1's time column only; a lost row or
row chunk reaches all six gradients. A clock can only be taken from a neighbour where there are two time groups."""
import pytest
import torch

import critic_restatement as C
import update_restatement as R
from conftest import load_golden
from oracle import nets

D = torch.float64
FACTOR = 10.0


def _close(a, b, tol=1e-12):
    a, b = a.detach().to(D), b.detach().to(D)
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def _moved(mut, ref):
    return float((mut.detach().double() - ref.detach().double()).abs().max())


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


# ---- the restatement against the oracle, the golden and autograd --------------------------------------------------------
def _oracle64(counts, tpr, weights):
    w1, b1, w2, b2, w3, b3 = (w.double() for w in weights)
    nf = torch.zeros(counts.size(0), counts.size(1), 7, dtype=D)
    nf[:, :, 1] = counts.double()
    return nets.critic_value(nf, tpr.double().unsqueeze(1), w1, b1, w2, b2, w3.reshape(1, -1), b3).view(-1)


@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.ROW_CASES, ids=_ids(C.ROW_CASES))
def test_float64_forward_equals_the_oracle_in_float64(M, N, rpt, clock):
    c = C.row_case(M, N, rpt, clock)
    v, h1, h2 = C.critic64(c.counts, c.times_per_row(), c.weights)
    assert v.dtype == D and h1.shape == (M, 64) and h2.shape == (M, 64)
    _close(v, _oracle64(c.counts, c.times_per_row(), c.weights))


def test_forward_equals_the_golden():
    """The golden's inputs and weights: float64 restatement == float64 oracle to 1e-12. The golden VALUES are what the
    reference computed in fp32, so float64 can only meet them at fp32 accuracy: atol 1e-5, rtol 1e-6, the tolerance
    test_oracle_golden.py applies to the oracle itself."""
    g = load_golden("nets")
    w = [g[f"val__final_mlp__{i}__{p}"] for i in (0, 2, 4) for p in ("weight", "bias")]
    weights = (w[0], w[1], w[2], w[3], w[4].reshape(-1), w[5])
    for nf, tm, val in ((g["node_features"].unsqueeze(0), g["time"].view(1), g["value"].view(1)),
                        (g["node_features_b"], g["time_b"].view(-1), g["value_b"].view(-1))):
        v64, _, _ = C.critic64(nf[:, :, 1], tm, weights)
        _close(v64, nets.critic_value(nf.double(), tm.double().unsqueeze(1), *(t.double() for t in w)).view(-1))
        assert torch.allclose(v64, val.double(), atol=1e-5, rtol=1e-6)
        v32, _, _ = C.critic32(nf[:, :, 1], tm, weights)
        assert torch.allclose(v32, val, atol=1e-5, rtol=1e-6)


@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.BWD_CASES, ids=_ids(C.BWD_CASES))
def test_manual_backward_equals_float64_autograd(M, N, rpt, clock):
    c = C.bwd_case(M, N, rpt, clock)
    ws = [w.double().requires_grad_(True) for w in c.weights]
    v, h1, h2 = C.critic64(c.counts, c.times_per_row(), ws)
    (v * c.grad_value.double()).sum().backward()
    got = C.critic_bwd64(c.counts, c.times_per_row(), c.weights, h1.detach(), h2.detach(), c.grad_value)
    for name, g, w in zip(C.GRAD_NAMES, got, ws):
        assert g.dtype == D and float(w.grad.abs().max()) > 0, name
        _close(g, w.grad.reshape(g.shape))


# ---- k_split_w1 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("S,N,Rr", C.SLAB_CASES, ids=_ids(C.SLAB_CASES))
def test_split_pieces_sum_to_w1_exactly(S, N, Rr, clock):
    c = C.slab_case(S, N, Rr, clock)
    w1 = c.weights[0]
    bits = C.split_w1(w1)
    K = C.kpad(N)
    assert bits.dtype.name == "uint16" and bits.shape == (3, 64, K) and K % 32 == 0 and 0 <= K - N < 32
    p = C.split_pieces64(w1)
    assert torch.equal(p.sum(0)[:, :N], w1[:, :N].double())           # every weight, exactly
    assert not bits[:, :, N:].any()                                    # zero padding
    assert bool((p[1] != 0).any()) and bool((p[2] != 0).any())
    # each piece is a bf16 (8 significant bits) and within half an ulp of what it rounds
    assert bool((p[1].abs() <= p[0].abs() * 2.0 ** -8).all()) and bool((p[2].abs() <= p[1].abs() * 2.0 ** -8 + 1e-300).all())
    tpr = c.times_per_row()
    full, _, _ = C.critic_pieces64(c.counts, tpr, c.weights)
    assert torch.equal(full, C.critic64(c.counts, tpr, c.weights)[0])


def test_bf16_rounding_is_to_nearest_even():
    import numpy as np
    x = np.array([1.0, 1.00390625, 1.01171875, 1.00390625 + 2.0 ** -23, -1.00390625, 0.0, 3.140625], dtype=np.float32)
    # 1 + 2^-8 is a tie -> even (1.0); 1 + 3 * 2^-8 is a tie -> even (1 + 2^-6); just above a tie rounds up
    want = np.array([1.0, 1.0, 1.015625, 1.0078125, -1.0, 0.0, 3.140625], dtype=np.float32)
    assert np.array_equal(C._bf16_bits_to_f32(C._bf16_rne_bits(x)), want)
    t = torch.from_numpy(x)
    assert np.array_equal(C._bf16_bits_to_f32(C._bf16_rne_bits(x)), t.bfloat16().float().numpy())


# ---- the launcher's rule and the case lists ------------------------------------------------------------------------------
def test_case_lists_reach_every_edge():
    ktiles = {n: (n + 31) // 32 for n in C.SLAB_N}
    assert sorted(ktiles.values()) == [1, 1, 1, 1, 2, 2, 3, 4, 4, 4, 5, 5] and {n % 32 for n in C.SLAB_N} == {0, 1, 3, 31}
    assert all((3, n, 128) in C.SLAB_CASES for n in C.SLAB_N)
    assert all((3, n, r) in C.SLAB_CASES for n in (1, 33, 128, 160) for r in (128, 256, 384, 512))
    assert {s for s, _, _ in C.SLAB_CASES} == {1, 3} and max(s * n * r for s, n, r in C.SLAB_CASES) == 3 * 160 * 512
    # wide tiles: honoured where the slab divides, silently 1 at R = 384; one workgroup == one whole slab at 256 / 2, 512 / 4
    assert [C.launched_ct(384, 3 * 384, ct) for ct in C.CTS] == [1, 1, 1]
    assert [C.launched_ct(256, 3 * 256, ct) for ct in C.CTS] == [1, 2, 1]
    assert [C.launched_ct(512, 3 * 512, ct) for ct in C.CTS] == [1, 2, 4]
    assert [C.launched_ct(128, 3 * 128, ct) for ct in C.CTS] == [1, 1, 1]
    for vals, col in (((1, 31, 32, 33, 127, 128, 129, 257), 0), ((1, 31, 32, 33, 63, 64, 65, 130), 1)):
        for v in vals:
            assert sum(1 for c in C.ROW_CASES if c[col] == v) >= 2, (col, v)
    assert {c[2] for c in C.ROW_CASES} == {1, 3} and any(c[2] == 3 and c[0] % 3 for c in C.ROW_CASES)
    assert {c[0] for c in C.BWD_CASES} == {1, 33, 511, 512, 513, 640, 777} and {c[1] for c in C.BWD_CASES} == {1, 63, 64, 65, 130}
    assert all((m, 65, 5) in C.BWD_CASES for m in (511, 512, 513)) and {c[2] for c in C.BWD_CASES} == {1, 5}
    assert any(c[2] == 5 and c[0] % 5 for c in C.BWD_CASES)
    for M, N, _ in C.ROW_CASES + C.BWD_CASES:
        assert M * (N + C.ROW_PAD) * 4 < 1 << 20          # launch-bound: under 1 MB of input


def test_inputs_hold_the_planted_bytes_and_distinct_clocks():
    for clock in C.CLOCKS:
        c = C.slab_case(3, 33, 256, clock)
        assert int(c.counts[0, 0]) == 0 and int(c.counts[0, -1]) == 255 and int(c.counts[-1, 0]) == 255 and int(c.counts[-1, -1]) == 0
        assert int(c.counts.max()) == 255 and int(c.counts.min()) == 0 and c.times.unique().numel() == 3
        assert torch.equal(c.slab_counts(3, 256)[1, :, 5], c.counts[256 + 5])
        b = C.bwd_case(777, 1, 1, clock)
        assert b.times.unique().numel() == 777 and torch.equal(b.times.double().float(), b.times)
        same = C.bwd_case(777, 1, 1, clock)
        assert torch.equal(b.counts, same.counts) and torch.equal(b.times, same.times)       # a function of the shape
    assert float(C.slab_case(1, 32, 128, "day").times[0]) >= 21540.0 and float(C.slab_case(1, 32, 128, "unit").times[0]) < 32.0


# ---- sensitivity of the forward cases ------------------------------------------------------------------------------------
def _forward_sensitivity(c, names, u8x3):
    tpr = c.times_per_row()
    ref = C.critic64(c.counts, tpr, c.weights)
    f32 = C.critic32(c.counts, tpr, c.weights)
    bound = [R.tensor_bound(R.max_err(f, r), r) for f, r in zip(f32, ref)]
    muts = {"last column": C.critic64(C.drop_column(c.counts, c.N - 1), tpr, c.weights),
            "first column": C.critic64(C.drop_column(c.counts, 0), tpr, c.weights)}
    if c.clock == "unit":
        # (not at the seconds-of-day scale: there the time column dominates the first layer and the fp32 error of the
        # reference itself, hence the bound, is of the order of what one count moves)
        muts["byte off by one"] = C.critic64(C.byte_off_by_one(c.counts)[0], tpr, c.weights)
    if c.G > 1:
        muts["neighbour's clock"] = C.critic64(c.counts, c.times_per_row(C.neighbour_clock(c.times)), c.weights)
    if u8x3:
        muts["mid piece"] = C.critic_pieces64(c.counts, tpr, c.weights, pieces=(0, 2))
    for what, mut in muts.items():
        for i, name in enumerate(names):
            moved = _moved(mut[i], ref[i])
            assert moved >= FACTOR * bound[i], (what, name, moved, bound[i], moved / bound[i])


@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("S,N,Rr", C.SLAB_CASES, ids=_ids(C.SLAB_CASES))
def test_slab_cases_notice_a_lost_column_byte_clock_or_piece(S, N, Rr, clock):
    _forward_sensitivity(C.slab_case(S, N, Rr, clock), ("value",), u8x3=True)


@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.ROW_CASES, ids=_ids(C.ROW_CASES))
def test_row_cases_notice_a_lost_column_byte_or_clock(M, N, rpt, clock):
    _forward_sensitivity(C.row_case(M, N, rpt, clock), ("value", "h1", "h2"), u8x3=False)


# ---- sensitivity of the backward cases -----------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.BWD_CASES, ids=_ids(C.BWD_CASES))
def test_backward_cases_notice_a_lost_row_chunk_column_byte_or_clock(M, N, rpt, clock):
    """h1 / h2 stand in for the device's: the fp32 forward of the CPU (the GPU test feeds the kernel's own)."""
    c = C.bwd_case(M, N, rpt, clock)
    tpr = c.times_per_row()
    _, h1, h2 = C.critic32(c.counts, tpr, c.weights)

    def bwd(counts=c.counts, times=tpr, gv=c.grad_value):
        return C.critic_bwd64(counts, times, c.weights, h1, h2, gv)

    ref = bwd()
    f32 = C.critic_bwd32(c.counts, tpr, c.weights, h1, h2, c.grad_value)
    bound = [R.tensor_bound(R.max_err(f, r), r, relative_scale=True) for f, r in zip(f32, ref)]

    def lost_from(row):
        gv = c.grad_value.clone()
        gv[row:] = 0
        return bwd(gv=gv)

    for i, name in enumerate(C.GRAD_NAMES):                        # the last row, all six
        moved = _moved(lost_from(M - 1)[i], ref[i])
        assert moved >= FACTOR * bound[i], ("last row", name, moved, bound[i])
    if M >= C.MANY_ROWS:                                           # the last chunk of the chunked form, ragged or not
        w1c = lost_from((M - 1) // C.W1_CHUNK * C.W1_CHUNK)
        small = lost_from((M - 1) // C.SMALL_CHUNK * C.SMALL_CHUNK)
        moved = _moved(w1c[0][:, :N], ref[0][:, :N])
        assert moved >= FACTOR * bound[0], ("last dW1 chunk", moved, bound[0])
        assert _moved(small[0][:, N], ref[0][:, N]) >= FACTOR * bound[0], "last small chunk, time column"
        for i in range(1, 6):
            assert _moved(small[i], ref[i]) >= FACTOR * bound[i], ("last small chunk", C.GRAD_NAMES[i])
    muts = {"last column": bwd(counts=C.drop_column(c.counts, N - 1)), "first column": bwd(counts=C.drop_column(c.counts, 0))}
    if clock == "unit":                                            # (see _forward_sensitivity)
        muts["byte off by one"] = bwd(counts=C.byte_off_by_one(c.counts)[0])
    for what, mut in muts.items():
        moved = _moved(mut[0][:, :N], ref[0][:, :N])
        assert moved >= FACTOR * bound[0], (what, moved, bound[0])
    if c.G > 1:
        moved = _moved(bwd(times=c.times_per_row(C.neighbour_clock(c.times)))[0][:, N], ref[0][:, N])
        assert moved >= FACTOR * bound[0], ("neighbour's clock", moved, bound[0])
