"""Float64 restatement of the critic MLP of csrc/critic.hip (MPNNValueNetSimple: cat(count per node, time) -> 64 -> 64 -> 1
with ReLU), of its backward with the kernel's contract, and a bit-level emulation of k_split_w1 (TEST INFRASTRUCTURE: plain
torch / numpy on the CPU, no kernel involved). ``test_critic_host.py`` pins it to ``oracle/nets.critic_value``, the
reference's golden and float64 autograd; ``test_gpu_critic_fp64.py`` compares every critic kernel with it. It also holds the
inputs of those GPU cases, so that the host test can check — without a GPU — that every case would notice a lost column,
row, chunk, clock or weight piece by more than 10x the tolerance the GPU test applies (``update_restatement.tensor_bound``).

Weights are ``final_mlp.{0,2,4}.{weight,bias}`` as the kernels take them: w1 (64, N + 1) with the time column last, b1 (64,),
w2 (64, 64), b2 (64,), w3 (64,), b3 (1,)."""
from __future__ import annotations

import numpy as np
import torch

H = 64              # hidden width (CR_H)
BK = 32             # k-tile of the slab kernels (CR_BK): k_split_w1 pads W1 to a multiple of it
BM = 128            # rows per MFMA tile (CR_BM)
MANY_ROWS = 512     # CB_MANY_ROWS: from this many rows on the chunked backward runs
W1_CHUNK = 128      # CB_RC: rows per chunk of the chunked dW1 pass
SMALL_CHUNK = 32    # CB_RS: rows per chunk of the chunked small-gradient pass
GRAD_NAMES = ("gw1", "gb1", "gw2", "gb2", "gw3", "gb3")


# ---- forward ---------------------------------------------------------------------------------------------------------------
def critic_fwd(counts, times_per_row, weights, dtype):
    """-> (value (M,), h1 (M, 64), h2 (M, 64)) computed in ``dtype``; counts (M, N) of any dtype, times_per_row (M,)."""
    w1, b1, w2, b2, w3, b3 = (w.to(dtype) for w in weights)
    x, t = counts.to(dtype), times_per_row.to(dtype)
    N = x.size(1)
    h1 = torch.relu(x @ w1[:, :N].t() + t.unsqueeze(1) * w1[:, N] + b1)
    h2 = torch.relu(h1 @ w2.t() + b2)
    return h2 @ w3.reshape(-1) + b3.reshape(()), h1, h2


def critic64(counts, times_per_row, weights):
    return critic_fwd(counts, times_per_row, weights, torch.float64)


def critic32(counts, times_per_row, weights):
    """The same arithmetic in fp32 on the CPU: its distance from ``critic64`` is the e32 that ``tensor_bound`` takes."""
    return critic_fwd(counts, times_per_row, weights, torch.float32)


# ---- backward with the kernel's contract -----------------------------------------------------------------------------------
def critic_bwd(counts, times_per_row, weights, h1, h2, grad_value, dtype):
    """The six gradients of sum(value * grad_value) from GIVEN activations: the ReLU masks are ``h > 0`` of the tensors passed
    in (tarl_critic_mlp_bwd takes h1 / h2 as inputs and never recomputes them), and dW2 / dW3 multiply by those tensors."""
    w1, _, w2, _, w3, _ = (w.to(dtype) for w in weights)
    x, t, gv = counts.to(dtype), times_per_row.to(dtype), grad_value.to(dtype)
    h1, h2 = h1.to(dtype), h2.to(dtype)
    dh2 = (h2 > 0).to(dtype) * gv.unsqueeze(1) * w3.reshape(1, -1)
    dh1 = (h1 > 0).to(dtype) * (dh2 @ w2)
    gw1 = torch.cat([dh1.t() @ x, (dh1 * t.unsqueeze(1)).sum(0).unsqueeze(1)], dim=1)
    return gw1, dh1.sum(0), dh2.t() @ h1, dh2.sum(0), h2.t() @ gv, gv.sum().reshape(1)


def critic_bwd64(counts, times_per_row, weights, h1, h2, grad_value):
    return critic_bwd(counts, times_per_row, weights, h1, h2, grad_value, torch.float64)


def critic_bwd32(counts, times_per_row, weights, h1, h2, grad_value):
    return critic_bwd(counts, times_per_row, weights, h1, h2, grad_value, torch.float32)


# ---- k_split_w1, bit for bit -----------------------------------------------------------------------------------------------
def _bf16_rne_bits(f32):
    """cr_bf16_rne: round-to-nearest-even bf16 of an fp32 array, as uint16 bit patterns."""
    u = np.ascontiguousarray(f32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def _bf16_bits_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def kpad(N):
    return (N + BK - 1) // BK * BK


def split_w1(w1):
    """w1 (64, N + 1) fp32 -> uint16 [3][64][Kpad]: hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid) of the count
    columns (the time column is not split), columns N .. Kpad - 1 zero. Every subtraction in fp32, as the kernel does them."""
    w1 = w1.detach().cpu().numpy().astype(np.float32)
    N = w1.shape[1] - 1
    w = np.zeros((H, kpad(N)), dtype=np.float32)
    w[:, :N] = w1[:, :N]
    hi = _bf16_rne_bits(w)
    r1 = (w - _bf16_bits_to_f32(hi)).astype(np.float32)
    mid = _bf16_rne_bits(r1)
    r2 = (r1 - _bf16_bits_to_f32(mid)).astype(np.float32)
    lo = _bf16_rne_bits(r2)
    return np.stack([hi, mid, lo])


def split_pieces64(w1):
    """The three pieces as float64 tensors (3, 64, Kpad)."""
    return torch.from_numpy(_bf16_bits_to_f32(split_w1(w1)).astype(np.float64))


def critic_pieces64(counts, times_per_row, weights, pieces=(0, 1, 2)):
    """``critic64`` with the count columns of W1 replaced by the sum of the chosen bf16 pieces (all three: W1 itself)."""
    w1 = weights[0]
    N = w1.size(1) - 1
    p = split_pieces64(w1)
    w1p = w1.double().clone()
    w1p[:, :N] = sum(p[i] for i in pieces)[:, :N]
    return critic64(counts, times_per_row, (w1p,) + tuple(weights[1:]))


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------
CLOCKS = ("unit", "day")
# (S slabs, N nodes, R environments per slab): every N at (3, N, 128) — 1, 1, 1, 1, 2, 2, 3, 4, 4, 4, 5, 5 k-tiles, N mod 32 in
# {0, 1, 3, 31} —; N in {1, 33, 128, 160} at every R: 256 and 512 are one whole slab per workgroup at CT = 2 and 4, 384 takes no
# wide tile; two single-slab cases
SLAB_N = (1, 3, 31, 32, 33, 64, 96, 97, 127, 128, 129, 160)
SLAB_CASES = tuple([(3, n, 128) for n in SLAB_N] + [(3, n, r) for n in (1, 33, 128, 160) for r in (256, 384, 512)] +
                   [(1, 32, 128), (1, 97, 128)])
CTS = (1, 2, 4)
# (M rows, N, rows_per_time): M and N on either side of split-K's 32-row block and 64-column chunk and of the 128-row MFMA tile
ROW_PAD = 12            # row stride = N + ROW_PAD
ROW_CASES = ((1, 1, 1), (1, 64, 3), (31, 31, 3), (31, 130, 1), (32, 32, 1), (32, 65, 3), (33, 33, 3), (33, 63, 1),
             (127, 64, 1), (127, 1, 3), (128, 130, 3), (128, 31, 1), (129, 65, 1), (129, 32, 3), (257, 63, 3), (257, 33, 1))
# (M, N, rows_per_time): 511 / 512 / 513 around CB_MANY_ROWS, N around the 64-column tile of the chunked dW1 pass
BWD_CASES = ((1, 1, 1), (1, 65, 5), (33, 63, 5), (33, 130, 1), (511, 65, 5), (512, 65, 5), (513, 65, 5), (511, 1, 1),
             (513, 64, 1), (640, 63, 1), (640, 130, 5), (777, 64, 5), (777, 1, 1), (512, 130, 1))


def launched_ct(R, M, requested):
    """The rule of tarl_critic_mlp_fwd_slabs_u8: TARL_CRITIC_CT is honoured when the slab is a whole number of 128 CT-row
    workgroups, else the default holds — 2 for slabs of a multiple of 256 rows from 1 024 workgroups on, else 1."""
    ct = 2 if R % (2 * BM) == 0 and M // (2 * BM) >= 1024 else 1
    if requested in CTS and R % (requested * BM) == 0:
        ct = requested
    return ct


def make_weights(N, gen):
    """nn.Linear's default initialisation (uniform on +-1 / sqrt(fan_in), weights and biases), from ``gen``."""
    def u(shape, fan_in):
        return ((torch.rand(shape, generator=gen) * 2 - 1) / fan_in ** 0.5).float()
    return (u((H, N + 1), N + 1), u((H,), N + 1), u((H, H), H), u((H,), H), u((H,), H), u((1,), H))


def make_counts(M, N, gen):
    """(M, N) bytes uniform on 0..255 with 0 and 255 planted in the first and last row and the first and last column."""
    c = torch.randint(0, 256, (M, N), generator=gen).to(torch.uint8)
    c[0, 0], c[M - 1, 0], c[0, N - 1] = 0, 255, 255
    if M > 1 and N > 1:
        c[M - 1, N - 1] = 0
    return c


def make_clocks(G, clock, gen):
    """One clock per time group. unit: 21.54 + 10 U. day: 21 540 + frame, seconds of the day as the trainer feeds them, the
    groups' frames distinct and not in order (a minibatch's rows come from shuffled frames)."""
    if clock == "unit":
        return (21.54 + 10.0 * torch.rand(G, generator=gen)).float()
    assert G < 1009
    frames = (torch.arange(G) * 37 + 11) % 1009         # distinct for G < 1009 (a prime)
    return (21540.0 + frames.float()).float()


# Cases whose first inputs failed a 10x sensitivity check of test_critic_host.py ON THE REFERENCE ALONE (no kernel involved); the
# inputs were changed, never the factor.
# - (family, M, N, clock) -> seed offset. Slab 3 x 160 x 256, unit clocks: the middle row's value moved by 0.7x the bound for one
#   count more in its middle column (the paths through the three layers cancelled for that row and column; 20x and more
#   elsewhere); slab 3 x 160 x 512, unit clocks: 14x, too close to the factor to hold on another CPU's fp32 matrix product.
RESEED = {("slab", 3 * 256, 160, "unit"): 1, ("slab", 3 * 512, 160, "unit"): 2}
# - (family, N, clock) -> factor on W1's time column. With one or three count columns and the clock in seconds of the day, the time
#   term (21 540 x a weight of the size of the count weights) sets the fp32 error of the reference: dropping the mid piece moved the
#   value by 1.7 .. 6x the bound only. A time weight of 1/32 the default (a power of two: nothing else about the numbers changes)
#   leaves the clock the largest term (670 against 255 per unit weight) and the mid piece visible.
TIME_WEIGHT_SCALE = {("slab", 1, "day"): 2.0 ** -5, ("slab", 3, "day"): 2.0 ** -5}


class Case:
    """Inputs of one case: counts (M, N) bytes in row order (row = slab * R + environment for the slab cases), one clock per
    time group, the six weights, a gradient seed per row. The seed is a function of the shape."""

    def __init__(self, family, M, N, rows_per_time, clock):
        seed = {"slab": 1, "rows": 2, "bwd": 3}[family] * 10 ** 7 + M * 1000 + N * 7 + rows_per_time + CLOCKS.index(clock) * 500009
        gen = torch.Generator().manual_seed(seed + RESEED.get((family, M, N, clock), 0))
        self.M, self.N, self.rpt, self.clock = M, N, rows_per_time, clock
        self.weights = make_weights(N, gen)
        self.weights[0][:, N] *= TIME_WEIGHT_SCALE.get((family, N, clock), 1.0)
        self.counts = make_counts(M, N, gen)
        self.G = (M + rows_per_time - 1) // rows_per_time
        self.times = make_clocks(self.G, clock, gen)
        self.grad_value = torch.randn(M, generator=gen).float()
        for m in (M // 2, M - 1):           # the rows the sensitivity checks mutate are never negligible ones
            self.grad_value[m] = 1.5 if self.grad_value[m] >= 0 else -1.5

    def times_per_row(self, times=None):
        return (self.times if times is None else times).repeat_interleave(self.rpt)[:self.M]

    def slab_counts(self, S, R):
        """(M, N) rows -> the env-minor rollout layout [S][N][R]."""
        return self.counts.view(S, R, self.N).permute(0, 2, 1).contiguous()


def slab_case(S, N, R, clock):
    return Case("slab", S * R, N, R, clock)


def row_case(M, N, rpt, clock):
    return Case("rows", M, N, rpt, clock)


def bwd_case(M, N, rpt, clock):
    return Case("bwd", M, N, rpt, clock)


# ---- the mutations of the sensitivity checks -------------------------------------------------------------------------------
def drop_column(counts, k):
    c = counts.clone()
    c[:, k] = 0
    return c


def byte_off_by_one(counts):
    """One count byte of the middle row, middle column, moved by one."""
    c = counts.clone()
    m, k = counts.size(0) // 2, counts.size(1) // 2
    c[m, k] = c[m, k] + 1 if int(c[m, k]) < 255 else 254
    return c, m


def neighbour_clock(times):
    """The last time group reads the clock of the group before it (a wrong ``gr / rows_per_time``)."""
    t = times.clone()
    t[-1] = t[-2]
    return t
