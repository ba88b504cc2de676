"""The single-kernel cases of the anti-aliased activation (csrc/oobleck.hip aa_act_kernel through ``sat_oobleck_unit`` kind AA_ACT;
tests/test_gpu_codec_antialias.py on the device, tests/test_codec_antialias_host.py on the CPU): shapes, seeded inputs, the float64
restatement on the operands the kernel sees, and the planted faults the gates of codec_units.gate_cl have to reject.

The operation, per channel along time (x of T rows, f the 12 taps of tests/golden/alias_free_standin.kaiser_sinc_filter1d in float64):
    u[m] = 2 sum_i xp[i] f[m + 15 - 2 i],  xp[i] = x[clamp(i - 5, 0, T - 1)],  m = 0 .. 2 T - 1
    v    = act(u)
    y[t] = sum_j f[j] v[clamp(2 t + j - 5, 0, 2 T - 1)]
``reference`` states the up step as the transposed convolution it is (row i of the padded input adds x f[j] at position 2 i + j - 15) and
the down step as a gather -- neither is the per-thread walk of the kernel, which scatters activated pairs into running sums.

Inputs follow tests/codec_units.py: batch 2, item 1 is ITEM1_SCALE times item 0, one input row of item 0 is all zeros."""
import os
import sys
import zlib

import torch

import codec_units as cu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import alias_free_standin as AF  # noqa: E402

TT = 32          # include/sat_hip.h: SAT_OOBLECK_AA_TIME_TILE (tests/test_codec_antialias_host.py holds the two together)
KIND = 11        # include/sat_hip.h: SAT_OOBLECK_UNIT_AA_ACT
# rows: the lengths at which the two clamps overlap (T < 6) or just do not (6), the golden length, and one row less / exactly / one row more
# than a time tile and two tiles plus three rows -- a wrong row at either end or at a tile seam is what these exist for.
# channels: 16 (48 pad channels), 64 (none), 192 (three 64-channel groups, none padded)
ROWS = [1, 2, 5, 6, 11, TT - 1, TT, TT + 1, 2 * TT + 3]
CHANNELS = [16, 64, 192]
ACTS = ["snake", "elu"]
CASES = [dict(c=c, rows=r, act=a) for a in ACTS for c in CHANNELS for r in ROWS]
FAULTS = ("zero_pad", "no_v_clamp", "no_gain", "phases_swapped", "drop_tap", "shift_row", "plain", "neighbour_alpha")
DROPPED_TAP = 4          # of the down filter: f[4] = 0.1286


def case_id(p):
    return f"{p['act']}-c{p['c']}-rows{p['rows']}"


def taps64():
    return AF.kaiser_sinc_filter1d(dtype=torch.float64).view(-1)


class Case:
    def __init__(self, p):
        self.p = dict(p)
        self.c, self.rows, self.act = p["c"], p["rows"], p["act"]
        gen = torch.Generator().manual_seed(zlib.crc32(repr(("aa_act", sorted(p.items()))).encode()))
        x = torch.randn((cu.BATCH, self.c, self.rows), generator=gen)
        x[1] *= cu.ITEM1_SCALE
        if self.rows > 4:
            x[0, :, 3] = 0.0
        self.x = x
        # log-scale Snake parameters wide enough that a neighbouring channel's alpha is another function: e^alpha in about 0.5 .. 2
        self.alpha = torch.randn((self.c,), generator=gen) * 0.4
        self.beta = torch.randn((self.c,), generator=gen) * 0.3

    def x_cl(self, fmt):
        """[b, t, Cp] in the operand type, pad channels zero: what the kernel is handed."""
        return fmt.round(cu.to_cl(self.x, cu.pad64(self.c))).to(fmt.dtype)


def reference(case, fmt, fault=None):
    """[b, t, Cp] float64: the activated tensor from the rounded input, pad channels zero.  ``fault`` plants one of FAULTS."""
    x = fmt.round(case.x).double()
    b, c, t = x.shape
    f = taps64()
    alpha = case.alpha.roll(1) if fault == "neighbour_alpha" else case.alpha
    act = lambda v: cu.activation(v, case.act, alpha, case.beta)
    if fault == "plain":
        return cu.to_cl(act(x), cu.pad64(c))
    rows = torch.arange(t + 10) - (4 if fault == "shift_row" else 5)
    xp = x[..., rows.clamp(0, t - 1)]
    if fault == "zero_pad":
        xp = xp * ((rows >= 0) & (rows < t)).double()
    u = x.new_zeros((b, c, 2 * t))
    for i in range(t + 10):
        for j in range(12):
            m = 2 * i + j - 15
            if 0 <= m < 2 * t:
                u[..., m] += f[j] * xp[..., i]
    if fault != "no_gain":
        u = 2.0 * u
    if fault == "phases_swapped":
        u = u.view(b, c, t, 2).flip(-1).reshape(b, c, 2 * t)
    v = act(u)
    g = f.clone()
    if fault == "drop_tap":
        g[DROPPED_TAP] = 0.0
    y = x.new_zeros((b, c, t))
    for j in range(12):
        m = 2 * torch.arange(t) + j - 5
        term = v[..., m.clamp(0, 2 * t - 1)]
        if fault in ("no_v_clamp", "zero_pad"):
            term = term * ((m >= 0) & (m < 2 * t)).double()
        y += g[j] * term
    return cu.to_cl(y, cu.pad64(c))


# What a fault cannot change, and why (the host test asserts the two results are equal there, and that every other pair is rejected):
#   T = 1: every row of the window is row 0 whatever the shift; u[0] = u[1] because the odd and the even taps of a symmetric filter have
#          the same sum (1 / 2), so swapping the phases moves nothing; and with 2 * 1 / 2 = 1 both are x[0], every v is act(x[0]) and the
#          down taps sum to 1: one row is a constant signal, which the filters pass unchanged, so the plain activation is the right answer
INVISIBLE = {("shift_row", 1), ("phases_swapped", 1), ("plain", 1)}
