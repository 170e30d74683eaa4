"""GPU: every kernel of csrc/critic.hip against the float64 restatement of tests/critic_restatement.py, at every tile and
chunk edge — the slab forwards (fp32, exact-chain bytes, the bf16 three-piece k_critic_fwd_slab_u8x3 at each tile width) from 1
to 5 k-tiles and N mod 32 in {0, 1, 3, 31}, with one, several and a fraction of a workgroup per slab; k_split_w1 bit for bit;
the row-major and split-K forwards around their 32 / 64 / 128 blocks, h1 and h2 included; the backward on either side of
CB_MANY_ROWS = 512 and of its 64-column tile, deterministic and inside its scratch.

Tolerances (none taken from a kernel): max(8 e32, 2^-22 scale) of update_restatement.tensor_bound, with e32 the error of the
same arithmetic in fp32 on the CPU; gradients with the relative scale. test_critic_host.py checks that each case here would
notice a lost column, byte, clock, weight piece, row or chunk by 10x that. Counts are bytes on 0..255, clocks at the unit and
at the seconds-of-day scale. Every buffer a kernel reads is followed by memory the test owns and has poisoned (bytes 255,
floats nan): a kernel that read past its rows would meet those, never foreign memory. Every case prints its e32, bound and
observed error."""
import numpy as np
import pytest
import torch

import critic_restatement as C
import update_restatement as R

pytestmark = pytest.mark.gpu
GUARD = 4096            # floats after the backward's scratch that must come back untouched


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tarl_hip import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


def _ids(cases):
    return ["x".join(str(v) for v in c) for c in cases]


def _cw(ops, weights):
    return ops.CriticWeights(*(dev(w.contiguous()) for w in weights))


def _check(what, got, ref, f32, relative_scale=False):
    """|got - ref| <= max(8 e32, 2^-22 scale) element by element, no element left out (nan fails)."""
    ref = ref.detach().double()
    got = got.detach().cpu().double().reshape(ref.shape)
    e32 = R.max_err(f32.detach(), ref)
    bound = R.tensor_bound(e32, ref, relative_scale)
    err = (got - ref).abs()
    worst = float(err.max()) if bool(torch.isfinite(err).all()) else float("nan")
    print(f"CRITIC {what}: e32 {e32:.3e} bound {bound:.3e} gpu {worst:.3e} ratio {worst / bound:.3f}")
    assert bool((err <= bound).all()), (what, worst, bound)


def _with_tail(t, fill, tail):
    """``t`` on the device, contiguous, followed by ``tail`` poisoned elements in the same allocation -> (view, whole buffer)."""
    buf = torch.full((t.numel() + tail,), fill, dtype=t.dtype, device="cuda")
    buf[:t.numel()] = dev(t).reshape(-1)
    return buf[:t.numel()].view(t.shape), buf


def _padded_rows(counts, dtype, fill, extra_rows=0):
    """(M, N) counts -> a (M, N) view of row stride N + ROW_PAD into a poisoned (M + extra_rows, N + ROW_PAD) buffer."""
    M, N = counts.shape
    big = torch.full((M + extra_rows, N + C.ROW_PAD), fill, dtype=dtype, device="cuda")
    big[:M, :N] = dev(counts).to(dtype)
    view = big[:M, :N]
    assert view.stride(0) == N + C.ROW_PAD
    return view


# ---- slab kernels and k_split_w1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("S,N,Rr", C.SLAB_CASES, ids=_ids(C.SLAB_CASES))
def test_slab_kernels_against_float64(ops, monkeypatch, S, N, Rr, clock):
    c = C.slab_case(S, N, Rr, clock)
    what = f"slab {S}x{N}x{Rr} {clock}"
    tpr = c.times_per_row()
    ref, f32 = C.critic64(c.counts, tpr, c.weights)[0], C.critic32(c.counts, tpr, c.weights)[0]
    cw, times = _cw(ops, c.weights), dev(c.times)
    slab = c.slab_counts(S, Rr)
    c8, buf8 = _with_tail(slab, 255, C.BK * Rr)
    cf, buff = _with_tail(slab.float(), float("nan"), C.BK * Rr)
    # fp32 slab == exact-chain bytes == the row-major kernel on the transposed rows, bit for bit
    v_f = ops.critic_forward_slabs(cw, cf, times)
    v_x = ops.critic_forward_slabs(cw, c8, times, exact_chain=True)
    v_r, _, _ = ops.critic_forward(cw, _padded_rows(c.counts, torch.float32, float("nan")), times, rows_per_time=Rr)
    assert torch.equal(v_f, v_x) and torch.equal(v_f, v_r)
    _check(what + " fp32 chain", v_f, ref, f32)
    # the bf16 three-piece kernel at each tile width: the launcher honours TARL_CRITIC_CT only where the slab is a whole number
    # of 128 CT-row workgroups (its rule, restated in critic_restatement.launched_ct: the library reports no kernel names)
    ran, v_ct = {}, {}
    for ct in C.CTS:
        monkeypatch.setenv("TARL_CRITIC_CT", str(ct))
        ran[ct] = C.launched_ct(Rr, S * Rr, ct)
        v_ct[ct] = ops.critic_forward_slabs(cw, c8, times)
        _check(what + f" u8x3 CT={ct} (ran {ran[ct]})", v_ct[ct], ref, f32)
    assert ran == {ct: (ct if Rr % (C.BM * ct) == 0 else 1) for ct in C.CTS}
    if Rr == 384:
        assert ran == {1: 1, 2: 1, 4: 1}                 # no wide tile divides the slab: the request falls back, silently
    if Rr == 512:
        assert ran == {1: 1, 2: 2, 4: 4}                 # (CT = 4: one workgroup is one whole slab)
    if Rr == 256:
        assert ran == {1: 1, 2: 2, 4: 1}                 # (CT = 2: one workgroup is one whole slab)
    assert torch.equal(v_ct[2], v_ct[1]) and torch.equal(v_ct[4], v_ct[1])
    # k_split_w1: the scratch the call leaves behind, written afresh (padding included) over a poisoned buffer
    scr = ops._SPLIT_SCRATCH[(str(c8.device), N)]
    K = C.kpad(N)
    assert scr.numel() == 3 * 64 * K * 2
    scr.fill_(0xA5)
    assert torch.equal(ops.critic_forward_slabs(cw, c8, times), v_ct[1])
    got = scr.cpu().numpy().view(np.uint16).reshape(3, 64, K)
    assert np.array_equal(got, C.split_w1(c.weights[0])), what + " split"
    # nothing wrote to the inputs or their tails
    assert torch.equal(c8.cpu(), slab) and bool((buf8[slab.numel():] == 255).all()) and bool(torch.isnan(buff[slab.numel():]).all())


# ---- row-major forward and split-K ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.ROW_CASES, ids=_ids(C.ROW_CASES))
def test_row_major_and_split_k_against_float64(ops, M, N, rpt, clock):
    c = C.row_case(M, N, rpt, clock)
    what = f"rows {M}x{N} rpt {rpt} {clock}"
    tpr = c.times_per_row()
    ref, f32 = C.critic64(c.counts, tpr, c.weights), C.critic32(c.counts, tpr, c.weights)
    cw, times = _cw(ops, c.weights), dev(c.times)
    xf = _padded_rows(c.counts, torch.float32, float("nan"))
    x8 = _padded_rows(c.counts, torch.uint8, 255)
    out_f = ops.critic_forward(cw, xf, times, rpt, keep_hidden=True)
    out_8 = ops.critic_forward(cw, x8, times, rpt, keep_hidden=True)
    out_k = ops.critic_forward(cw, xf, times, rpt, keep_hidden=True, split_k=True)
    out_k2 = ops.critic_forward(cw, xf, times, rpt, keep_hidden=True, split_k=True)
    for i, name in enumerate(("value", "h1", "h2")):
        _check(f"{what} mfma {name}", out_f[i], ref[i], f32[i])
        _check(f"{what} split-K {name}", out_k[i], ref[i], f32[i])
        assert torch.equal(out_8[i], out_f[i]), name + ": byte rows != fp32 rows"
        assert torch.equal(out_k2[i], out_k[i]), name + ": split-K differs between two calls"


# ---- backward ------------------------------------------------------------------------------------------------------------
def _backward(ops, cw, counts, times, rpt, h1, h2, gv, M, N):
    """tarl_critic_mlp_bwd into zeroed gradients, with a scratch of exactly tarl_critic_mlp_bwd_scratch_floats floats (nan: a
    partial sum read before it is written shows) followed by a guard the kernels must not touch."""
    from tarl_hip import lib
    L = lib.load()
    n = int(L.tarl_critic_mlp_bwd_scratch_floats(M, N))
    chunked = M >= C.MANY_ROWS
    parts = -(-M // C.W1_CHUNK) * 64 * N + -(-M // C.SMALL_CHUNK) * (64 * 64 + 4 * 64 + 1)
    assert n == 2 * M * 64 + (parts if chunked else 0)                    # which form runs, from M
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    buf[n:] = -1234.5
    grads = [torch.zeros_like(w) for w in (cw.w1, cw.b1, cw.w2, cw.b2, cw.w3, cw.b3)]
    lib.check(L.tarl_critic_mlp_bwd(counts.data_ptr(), counts.stride(0), M, N, times.data_ptr(), rpt, cw.w1.data_ptr(),
                                    cw.w2.data_ptr(), cw.w3.data_ptr(), h1.data_ptr(), h2.data_ptr(), gv.data_ptr(),
                                    buf.data_ptr(), *(g.data_ptr() for g in grads), lib.current_stream()))
    torch.cuda.synchronize()
    assert bool((buf[n:] == -1234.5).all()), "the backward wrote past its scratch"
    assert bool(torch.isfinite(buf[:n]).all()), "part of the scratch was never written"
    return grads


@pytest.mark.parametrize("clock", C.CLOCKS)
@pytest.mark.parametrize("M,N,rpt", C.BWD_CASES, ids=_ids(C.BWD_CASES))
def test_backward_against_float64(ops, M, N, rpt, clock):
    c = C.bwd_case(M, N, rpt, clock)
    what = f"bwd {M}x{N} rpt {rpt} {clock} ({'chunked' if M >= C.MANY_ROWS else 'small'})"
    tpr = c.times_per_row()
    cw, times, gv = _cw(ops, c.weights), dev(c.times), dev(c.grad_value)
    # a whole dW1 chunk of poisoned rows after the last one: what a chunk that ignored its row count would read
    xf = _padded_rows(c.counts, torch.float32, float("nan"), extra_rows=C.W1_CHUNK)
    _, h1, h2 = ops.critic_forward(cw, xf, times, rpt, keep_hidden=True)
    # the reference works from the device's own activations: a unit within rounding of 0 cannot flip a mask
    ref = C.critic_bwd64(c.counts, tpr, c.weights, h1.cpu(), h2.cpu(), c.grad_value)
    f32 = C.critic_bwd32(c.counts, tpr, c.weights, h1.cpu(), h2.cpu(), c.grad_value)
    g1 = _backward(ops, cw, xf, times, rpt, h1, h2, gv, M, N)
    g2 = _backward(ops, cw, xf, times, rpt, h1, h2, gv, M, N)
    for name, a, b, r, f in zip(C.GRAD_NAMES, g1, g2, ref, f32):
        _check(f"{what} {name}", a, r, f, relative_scale=True)
        assert torch.equal(a, b), name + " differs between two calls"        # fixed summation order, no atomics
    # the library's own entry point (its scratch, accumulating into zeros) gives the same bits
    g3 = [torch.zeros_like(g) for g in g1]
    ops.critic_backward(cw, xf, times, rpt, h1, h2, gv, g3)
    assert all(torch.equal(a, b) for a, b in zip(g1, g3))
