"""Shared helpers for the parity tests."""
import torch


def rel_l2(a, b):
    a = a.detach().float().cpu()
    b = b.detach().float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def max_abs(a, b):
    return (a.detach().float().cpu() - b.detach().float().cpu()).abs().max().item()


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def assert_close(name, got, want, tol):
    err = rel_l2(got, want)
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite values in the HIP result"
    assert err <= tol, f"{name}: rel-L2 {err:.3e} > tol {tol:.1e} (max abs {max_abs(got, want):.3e})"
    return err


def fp16_round(x):
    return x.clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float32)


class OperandFormat:
    """The two 16-bit operand formats of the matrix kernels (sat_dit_cfg.gemm_dtype 0 / 3): torch dtype, the rounding the kernels
    apply at their store points, the C-ABI name mapping (sat_*_bf16* -> sat_*_f16*), and the share of a bf16 tolerance that the
    format's unit roundoff leaves (bf16 2^-9, fp16 2^-12: gates for fp16 are the bf16 gates / 4, a 2x margin on the 8x)."""

    def __init__(self, name):
        self.name = name
        self.f16 = name == "f16"
        self.dtype = torch.float16 if self.f16 else torch.bfloat16
        self.round = fp16_round if self.f16 else bf16_round
        self.tol_scale = 0.25 if self.f16 else 1.0
        self.gemm_dtype = "fp16" if self.f16 else "bf16"          # the name set_gemm_dtype / SAT_GEMM_DTYPE use

    def fn(self, lib, name):
        return getattr(lib, name.replace("bf16", "f16") if self.f16 else name)

    def tol(self, bf16_tol):
        return bf16_tol * self.tol_scale

    def __repr__(self):
        return self.name


FORMATS = [OperandFormat("bf16"), OperandFormat("f16")]

# The operand format every test that is not parametrised over FORMATS runs in: the PACKAGE DEFAULT ("fp16", what a user gets) unless
# SAT_TEST_DTYPE=bf16 selects the other build (tools/gpu_session.sh runs the suite under both).  Gates written as T(x) = SUITE.tol(x) are
# the bf16 gates of rounds 1-3 (~2x the error measured on MI355X), divided by 4 under fp16.
import os as _os

_suite_name = _os.environ.get("SAT_TEST_DTYPE", "fp16")
assert _suite_name in ("fp16", "bf16"), f"SAT_TEST_DTYPE must be fp16 or bf16, got {_suite_name!r}"
SUITE = FORMATS[1] if _suite_name == "fp16" else FORMATS[0]


# ---------------------------------------------------------------------------------------------------------------- sliced gates
# assert_close takes one rel-L2 figure over the whole tensor: right for rounding noise, blind to what kernels get wrong -- one tail row,
# one 32 x 32 accumulator block, one head of one query, a mask edge (diluted by every correct slice around it).  The sliced gate applies
# the same tolerance to every slice on its own.
def _f64(x):
    return x.detach().to("cpu", torch.float64)


def slice_errors(got, want, keep_dims):
    """One error per slice: the dimensions in keep_dims index the slices, every other dimension is reduced.
    err_s = ||got_s - want_s|| / max(||want_s||, rms over all slices of ||want_s||) -- the floor keeps near-zero slices from blowing up.
    A slice with a non-finite element has a non-finite error (and fails every gate).  Returns a float64 tensor of the kept shape."""
    got, want = _f64(got), _f64(want)
    assert got.shape == want.shape, f"shape mismatch: {tuple(got.shape)} vs {tuple(want.shape)}"
    keep = tuple(d % want.dim() for d in keep_dims)
    red = tuple(d for d in range(want.dim()) if d not in keep)
    if not red:
        num, den = (got - want).abs(), want.abs()
    else:
        num = (got - want).pow(2).sum(dim=red).sqrt()
        den = want.pow(2).sum(dim=red).sqrt()
    floor = den.pow(2).mean().sqrt().clamp_min(1e-300)
    return num / torch.maximum(den, floor)


def blocks32(x):
    """[m, n] -> [ceil(m/32), 32, ceil(n/32), 32] (keep_dims (0, 2): one slice per 32-row x 32-column block, the MFMA accumulator block).
    The ragged edge is padded with zeros, which add nothing to either norm: partial blocks are slices of their own."""
    x = _f64(x)
    m, n = x.shape
    mp, np_ = (m + 31) // 32 * 32, (n + 31) // 32 * 32
    out = torch.zeros((mp, np_), dtype=x.dtype)
    out[:m, :n] = x
    return out.view(mp // 32, 32, np_ // 32, 32)


def slice_spread(want, keep_dims, out_round):
    """F_ref: how far the worst slice of a correctly rounded result sits above its whole-tensor figure -- the largest slice error of
    out_round(want) against want over that pair's rel-L2.  From the reference alone; 1 for fp32 outputs (out_round None)."""
    if out_round is None:
        return 1.0
    want = _f64(want)
    rounded = _f64(out_round(want.float()))
    whole = ((rounded - want).norm() / want.norm().clamp_min(1e-300)).item()
    if whole == 0.0:
        return 1.0
    return max(1.0, slice_errors(rounded, want, keep_dims).max().item() / whole)


PARITY_LOG = _os.environ.get("SAT_PARITY_LOG")          # a file that collects one line per sliced assertion (profiles/parity_gates.txt)


def _log_gate(name, whole, worst, idx, f_ref, gate, slices):
    if PARITY_LOG:
        test = _os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(PARITY_LOG, "a") as f:
            f.write(f"{test}\t{name}\twhole={whole:.3e}\tworst={worst:.3e}\tat={idx}\tslices={slices}\tF_ref={f_ref:.3f}\tgate={gate:.3e}\n")


def assert_close_sliced(name, got, want, tol, keep_dims, out_round=None):
    """The companion of assert_close(name, got, want, tol): every slice (slice_errors) has to pass tol * max(1, F_ref), F_ref the spread of
    the output rounding's own noise over these slices (slice_spread).  Returns (worst slice error, its index, F_ref, gate)."""
    errs = slice_errors(got, want, keep_dims)
    f_ref = slice_spread(want, keep_dims, out_round)
    gate = tol * max(1.0, f_ref)
    flat = errs.reshape(-1)
    bad = ~(flat <= gate)                                       # (a NaN error is bad)
    pos = int(torch.nan_to_num(flat, nan=float("inf"), posinf=float("inf")).argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(pos), errs.shape)) if errs.dim() else ()
    worst = flat[pos].item()
    whole = rel_l2(got, want)
    _log_gate(name, whole, worst, idx, f_ref, gate, flat.numel())
    assert not bool(bad.any()), (f"{name}: slice {idx} (dims {tuple(keep_dims)}) has error {worst:.3e} > gate {gate:.3e} "
                                 f"(tol {tol:.1e} x F_ref {f_ref:.2f}); {int(bad.sum())} of {flat.numel()} slices fail, whole-tensor rel-L2 {whole:.3e}")
    return worst, idx, f_ref, gate


def assert_close_rows_blocks(name, got, want, tol, out_round=None):
    """[m, n] outputs of the row kernels and the GEMMs: gated per row and per 32 x 32 accumulator block."""
    assert_close_sliced(name + " per row", got, want, tol, (0,), out_round)
    assert_close_sliced(name + " per 32x32 block", blocks32(got), blocks32(want), tol, (0, 2), out_round)


# ---------------------------------------------------------------------------------------------------- sentinel outputs, guard bands
_SENTINEL_BYTE = 0xA5
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class Guarded:
    """An output buffer inside a larger sentinel-filled allocation: ``.t`` (the interior view; pass its pointer to the kernel) starts
    256-byte aligned, with at least 256 rows of the output's row pitch (the tallest tile) of guard on each side -- ``pitch``, in elements,
    where one row of the kernel is more than the last dimension (ln_part [m, d / 64, 2]: 2 * d / 64) or the output is flat.  Floating buffers are
    filled with NaN, integer ones with 0xA5 bytes; ``init`` (a residual the kernel accumulates into) fills the interior only.  After the
    call, check() wants the guards bit-identical to the sentinel and assert_written() every interior element finite: a kernel that
    skips a tail tile cannot pass on what the allocator left in the block, one that writes past its output cannot pass at all."""

    def __init__(self, shape, dtype, device, init=None, name="output", pitch=None):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        item = torch.empty((), dtype=dtype).element_size()
        guard = 256 * (pitch or shape[-1])
        self.guard = guard
        align = 256 // item
        raw = torch.empty(n + 2 * guard + 2 * align, dtype=dtype, device=device)
        off = guard + (-(raw.data_ptr() // item + guard)) % align
        assert raw.data_ptr() % item == 0 and (raw.data_ptr() + off * item) % 256 == 0 and off >= guard and raw.numel() - off - n >= guard
        self.name, self.n, self.off, self.raw = name, n, off, raw
        self.bits = _BITS[item]
        if dtype.is_floating_point:
            raw.fill_(float("nan"))
        else:
            raw.view(torch.uint8).fill_(_SENTINEL_BYTE)
        self.sentinel = int(raw[:1].view(self.bits).cpu().item())
        self.t = raw[off:off + n].view(shape)
        assert self.t.data_ptr() % 256 == 0 and self.t.is_contiguous()
        if init is not None:
            self.t.copy_(init)

    def check(self):
        """The guards are bit-identical to the sentinel: nothing was written outside the output."""
        for side, g, base in (("below", self.raw[:self.off], -self.off), ("above", self.raw[self.off + self.n:], self.n)):
            hit = (g.view(self.bits) != self.sentinel).nonzero()
            assert hit.numel() == 0, (f"{self.name}: {hit.shape[0]} guard elements {side} the output were overwritten, the first at element "
                                      f"{base + int(hit[0, 0])} relative to the output's start")
        return self

    def assert_written(self, region=None):
        """Every element of the interior (or of ``region``, a view of it) that the contract says is written is finite."""
        x = self.t if region is None else region
        assert x.dtype.is_floating_point, "byte outputs are compared against the reference instead"
        bad = ~torch.isfinite(x.float())
        if bool(bad.any()):
            first = tuple(int(i) for i in bad.nonzero()[0])
            raise AssertionError(f"{self.name}: {int(bad.sum())} elements of the output were left unwritten (sentinel NaN) or are non-finite, the first at {first}")
        return self


def guarded(shape, dtype, device, init=None, name="output", pitch=None):
    return Guarded(shape, dtype, device, init=init, name=name, pitch=pitch)


# --------------------------------------------------------------------------------------- bit equality, poisoned workspaces
# The output of a plan call is a pure function of weights and inputs (no atomics on the compute path, a bit-deterministic K-split reduce),
# so "does not depend on the workspace's bytes or on earlier calls" is asserted bit for bit: tests/test_gpu_state_independence.py.
NAN_BYTE = 0xFF
# byte -> why a uint8 workspace is filled with it before a call
WORKSPACE_FILLS = {
    0x00: "the baseline: what a pad reads as when somebody did clear it",
    NAN_BYTE: "a NaN in fp32, fp16, bf16, e4m3 and E8M0: any arithmetic on a stale element poisons the result",
    0x7B: "large but finite (61280 as fp16, about 1.3e36 as bf16 / fp32, 352 as e4m3): survives a max or a compare-based mask that drops a NaN",
    0x3C: "ordinary magnitude (about 1.06 as fp16, 0.0115 as bf16 / fp32): garbage that no range check would ever flag",
}


def fill_pattern(byte, dtype, n=1):
    """n elements of ``dtype`` whose every byte is ``byte``: what a filled uint8 workspace reads as in that format."""
    item = torch.empty((), dtype=dtype).element_size()
    return torch.full((n * item,), byte, dtype=torch.uint8).view(dtype)


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x if not x.dtype.is_floating_point and x.dtype != torch.bool else x.view(_BITS[x.element_size()])


def assert_bit_equal(name, got, want):
    """got and want hold the same bit patterns (compared as same-width integers on the CPU): +0.0 and -0.0 differ, two NaNs with the same
    bits are equal.  On failure: how many elements differ, the first differing index, both values there, the largest absolute difference."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    g, w = _bits(got), _bits(want)
    diff = g != w
    n = int(diff.sum())
    if n == 0:
        return
    flat = int(diff.reshape(-1).nonzero()[0, 0])
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), diff.shape)) if diff.dim() else ()
    gv, wv = got.detach().cpu().reshape(-1)[flat], want.detach().cpu().reshape(-1)[flat]
    d = (got.detach().cpu().double() - want.detach().cpu().double()).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)      # a NaN on one side only is as far off as it gets
    d = torch.where(diff, d, torch.zeros_like(d))
    raise AssertionError(f"{name}: {n} of {diff.numel()} elements differ in their bits, the first at {idx}: got {gv.item()!r} "
                         f"(0x{int(g.reshape(-1)[flat]) & (2 ** (8 * g.element_size()) - 1):x}), want {wv.item()!r} "
                         f"(0x{int(w.reshape(-1)[flat]) & (2 ** (8 * w.element_size()) - 1):x}); largest absolute difference {d.max().item():.3e}")


def e4m3_code_distance(got_bytes, want_bytes):
    """|distance in e4m3 codes| per element between two uint8 images (sign-magnitude order; +0 and -0 coincide)."""
    def order(b):
        b = b.detach().cpu().to(torch.int16)
        return torch.where(b >= 128, -(b - 128), b)
    return (order(got_bytes) - order(want_bytes)).abs()
