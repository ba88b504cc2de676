"""The single-kernel cases of the sampler, conditioning and audio I/O kernels of csrc/dit_glue.hip -- what runs outside the DiT blocks, in the
sampler loop and at the audio boundary: lincomb, dpmpp3m_update, inpaint_mix, dpm_error_partials, cfg_combine, vae_sample, snake_beta,
number_embed, float_to_int16, overlap_add and resample_sinc.  Shapes, seeded inputs, a restatement of every operation in plain PyTorch, and the
gates, in the pattern of fp32_units.py (whose helpers, tolerances and LOG this module shares).  The device test (test_gpu_sampler_kernels.py)
runs each entry of include/sat_hip.h and compares with ``reference(case)`` in float64; the host test (test_sampler_kernels_host.py) proves the
references against the oracle, shows that the same restatement evaluated in float32 on the CPU passes every gate, and that the gates reject the
faults these kernels can have.

``reference(case, dtype)`` is written from the header comment of each entry and from the lines of the reference project it cites, never from the
kernel, and is generic in the dtype: float64 is the reference, float32 the CPU evaluation.  For a linear form it also returns "<name>:mag" and
"<name>:n" of the a-priori bound.

Gates (``check``), none of them tuned on a kernel:
  linear forms   lincomb, dpmpp3m_update, the written half of inpaint_mix, overlap_add, resample_sinc, cfg_combine without the std rescale:
                 every element |got - want| <= (n + 4) 2^-24 mag, n the number of products in the formula as written and mag the float64 sum of
                 their magnitudes (a difference c (u - v) counts |c| |u| + |c| |v|; a plain addend counts its magnitude).  Any summation order,
                 with or without FMA contraction; not scaled by ``headroom``.  An element no product reaches (mag == 0) has to be exactly 0
  dpm_error      the float64 sum of the partials against the float64 reference under ``dpm_error_bound`` (derived there); every partial written,
                 finite and non-negative; the partials of blocks that own no element exactly 0.0
  transcendental snake_beta, vae_sample, number_embed, cfg_combine with the std rescale: |err| <= 1e-5 max(|want|, rms(want)) per element and
                 1e-5 per (batch, channel) row (per value row for number_embed); ``headroom`` scales these (0.25 for the CPU evaluation)
  exact          float_to_int16 equals x.div(div).mul(32767).to(int16) of the CPU, and silence gives zeros; the elements inpaint_mix keeps are
                 bit-identical to their input"""
import math

import torch
import torch.nn.functional as F

from fp32_units import LOG, MODEL_GATE, TOL, UNIT, _c, _gen, _note, _product, _rand, bound_share, case_id  # noqa: F401  (re-exported)
from util import assert_bit_equal, assert_close_sliced

GRID_CAP = 2048 * 256          # lincomb, dpmpp3m_update, inpaint_mix and both passes of float_to_int16 launch at most 2048 workgroups of 256
BIG = GRID_CAP + 257           # ... and stride beyond: a second pass of 257 elements, one full workgroup and a tail of one element
F64 = torch.float64

# ------------------------------------------------------------------------------------------------------------------------ the cases
_LC_COEF = (0.75, -1.3, 2.1, -0.4, 0.9)
# (a, b, c1, c2, cn) and which of d1 / d2 / noise are non-NULL, as sample_k hands them over (inference/sampling.py: have = 0, 1, 2 and the
# step onto sigma = 0, whose coefficients are (0, 1, 0, 0, 0) with both histories valid and no noise drawn)
DPMPP_STEPS = {
    "first": ((0.31, 0.69, 0.0, 0.0, 1.7), (0, 0, 1)),
    "second": ((0.42, 0.58, 0.21, 0.0, 0.9), (1, 0, 1)),
    "steady": ((0.55, 0.45, 0.33, -0.12, 0.4), (1, 1, 1)),
    "last": ((0.0, 1.0, 0.0, 0.0, 0.0), (1, 1, 0)),
}
_MIX_STEPS = [(3, 0), (3, 1), (3, 2), (7, 0), (7, 2), (7, 6), (100, 0), (100, 32), (100, 98)]
_MIX_BIG_T = -(-GRID_CAP // 3) + 257
VAE_PLANTED = (-100.0, -20.0, 0.0, 19.999, 20.0, 20.001, 60.0)
_OLA_SHAPES = [(1, 1, 1, 16, 16, 4), (2, 3, 2, 32, 24, 8), (1, 4, 1, 32, 32, 0), (1, 3, 1, 32, 40, 4), (2, 5, 2, 64, 48, 16)]
_RS_SHAPES = [(48000, 44100, 1, 1), (48000, 44100, 5, 159), (48000, 44100, 5, 161), (22050, 44100, 3, 100), (44100, 16000, 7, 883)]

CASES = {
    # 0, 1, 2, 3 and 5 terms (the NULL ones carry non-zero coefficients, the first of them NaN); one element, one wave short of a workgroup,
    # exactly one, one and an element, and the strided pass; out aliasing the first and the fourth term
    "lincomb": ([dict(n=257, terms=t, alias="-") for t in ("", "2", "03", "014", "01234")]
                + [dict(n=n, terms="024", alias="-") for n in (1, 255, 256, BIG)]
                + [dict(n=n, terms="01234", alias=a) for n in (257, BIG) for a in ("t0", "t3")]),
    "dpmpp3m_update": _product(n=[77, BIG], step=list(DPMPP_STEPS)),
    "inpaint_mix": ([dict(rows=r, t=t, steps=s, i=i) for (r, t) in ((1, 1), (16, 77)) for (s, i) in _MIX_STEPS]
                    + [dict(rows=3, t=_MIX_BIG_T, steps=s, i=i) for (s, i) in ((3, 0), (7, 2), (100, 98))]),
    "dpm_error_partials": (_product(n=[1, 1232, 256 * 64 + 5, BIG], parts=[1, 64, 1024, 4096], var=["mixed"])
                           + [dict(n=1232, parts=64, var="atol"), dict(n=1232, parts=64, var="rtol")]),
    "cfg_combine": [dict(b=b, c=c, t=t, phi=phi, scale=s) for (b, c, t) in ((1, 2, 1), (2, 8, 77), (3, 64, 257)) for phi in (0.0, 0.6)
                    for s in (1.0, 7.0)],
    "vae_sample": [dict(b=1, c=1, t=1, s=v) for v in VAE_PLANTED] + [dict(b=2, c=4, t=50, s="all"), dict(b=3, c=5, t=333, s="all")],
    "snake_beta": [dict(b=b, c=c, t=t, beta=be) for (b, c, t) in ((1, 1, 1), (3, 1, 7), (2, 5, 333), (1, 3, 1)) for be in (-30.0, 0.0, 3.0)],
    "number_embed": [dict(count=n, half=h, features=f) for n in (1, 5) for (h, f) in ((1, 1), (128, 768), (300, 257))],
    # peak below and above 1, both settings; the peak inside, or negative in the last element (the tail of the strided pass at BIG); silence
    "float_to_int16": ([dict(n=n, maximize=m, peak=pk, where=w) for (n, w) in ((1, "last"), (4099, "rand"), (4099, "last"), (BIG, "last"))
                        for m in (0, 1) for pk in (0.3, 2.5)] + [dict(n=4099, maximize=m, peak=0.0, where="zero") for m in (0, 1)]),
    # one chunk; three and five overlapping chunks of two channels and two items; no overlap at all; a gap between the chunks; each with the
    # output exactly as long as the chunks reach and 5 samples longer (nothing covers those)
    "overlap_add": [dict(batch=b, chunks=n, c=c, l=l, hop=h, ov=o, extra=e) for (b, n, c, l, h, o) in _OLA_SHAPES for e in (0, 5)],
    # 48 kHz -> 44.1 kHz is 160 -> 147 with 174 taps: one sample; 159 (one frame, 147 phases, the window runs past both ends); 161 (a second
    # frame of one phase); 1 -> 2 (15 taps); 441 -> 160 with 475 taps and 7 rows; and an output 3 samples short of the ceiling
    "resample_sinc": ([dict(orig_sr=o, new_sr=n, rows=r, in_len=l, short=0) for (o, n, r, l) in _RS_SHAPES]
                      + [dict(orig_sr=48000, new_sr=44100, rows=5, in_len=161, short=3)]),
}
KINDS = tuple(CASES)


def _f32(v):
    """The float32 image of a Python float, as a Python float: what a c_float argument holds."""
    return float(torch.tensor(v, dtype=torch.float32))


def mask_boundary(i, steps):
    """(below, at, above): the float32 of (i + 1) / steps and its two float32 neighbours."""
    at = torch.tensor((i + 1) / steps, dtype=torch.float32)
    inf = torch.tensor(math.inf)
    return float(torch.nextafter(at, -inf)), float(at), float(torch.nextafter(at, inf))


class Case:
    """kind + parameters -> seeded inputs ``t`` (CPU tensors) and the scalars ``dim`` the entry is called with (floats as their fp32 image)."""

    def __init__(self, kind, p):
        self.kind, self.p = kind, dict(p)
        self.name = f"{kind} {case_id(p)}"
        self.t, self.dim = {}, {}
        getattr(self, "_" + kind)(_gen(kind, p), self.p, self.t, self.dim)
        self.dim = {k: _f32(v) if isinstance(v, float) else v for k, v in self.dim.items()}

    def _lincomb(self, g, p, t, d):
        n = p["n"]
        null_seen = False
        coef = []
        for i in range(5):
            if str(i) in p["terms"]:
                t[f"t{i}"] = _rand(g, n) * (1.0 + i)
                coef.append(_LC_COEF[i])
            else:
                t[f"t{i}"] = None
                coef.append(_LC_COEF[i] if null_seen else math.nan)            # a NULL term is skipped whatever its coefficient
                null_seen = True
        d.update(n=n, coef=tuple(coef))

    def _dpmpp3m_update(self, g, p, t, d):
        n = p["n"]
        (a, b, c1, c2, cn), (h1, h2, hn) = DPMPP_STEPS[p["step"]]
        t["x"], t["d"] = _rand(g, n) * 3.0, _rand(g, n)
        t["d1"] = _rand(g, n) if h1 else None
        t["d2"] = _rand(g, n) if h2 else None
        t["noise"] = _rand(g, n) if hn else None
        d.update(n=n, a=a, b=b, c1=c1, c2=c2, cn=cn)

    def _inpaint_mix(self, g, p, t, d):
        rows, tt = p["rows"], p["t"]
        below, at, above = mask_boundary(p["i"], p["steps"])
        mask = torch.rand(tt, generator=g)
        if tt == 1:
            mask[0] = at
        else:
            # 0 and 1, the boundary and its neighbours at the front, in the middle and in the last three frames (at BIG the tail of the strided pass)
            mask[0], mask[1], mask[2], mask[3], mask[4] = 0.0, below, at, above, 1.0
            mid = tt // 2
            mask[mid], mask[mid + 1], mask[mid + 2] = above, at, below
            mask[tt - 4], mask[tt - 3], mask[tt - 2], mask[tt - 1] = 1.0, below, above, at
        t["mask"] = mask
        t["x"], t["init"], t["noise"] = _rand(g, rows, tt) * 3.0, _rand(g, rows, tt), _rand(g, rows, tt)
        d.update(rows=rows, t=tt, sigma=0.3 + 1.1 * p["i"] / p["steps"], strength=(p["i"] + 1) / p["steps"])

    def _dpm_error_partials(self, g, p, t, d):
        n = p["n"]
        atol, rtol = {"mixed": (0.01, 0.01), "atol": (0.5, 0.01), "rtol": (1e-6, 0.05)}[p["var"]]
        lo = _rand(g, n) * 2.0
        # |x_prev| is 3 x |x_low| in about half of the elements and 0.3 x in the others, with either sign
        prev = lo * torch.where(torch.rand(n, generator=g) < 0.5, 3.0, 0.3) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        hi = lo + 0.01 * _rand(g, n)
        if n > 1:            # the last element carries a tenth of the whole sum
            delta = torch.clamp(_f32(rtol) * torch.maximum(lo.abs(), prev.abs()).double(), min=_f32(atol))
            others = ((lo.double() - hi.double()) / delta)[:n - 1].pow(2).sum()
            hi[n - 1] = lo[n - 1] + (torch.sqrt(others / 9.0) * delta[n - 1]).float()
        t.update(x_low=lo, x_high=hi, x_prev=prev)
        d.update(n=n, parts=p["parts"], atol=atol, rtol=rtol)

    def _cfg_combine(self, g, p, t, d):
        b, c, tt = p["b"], p["c"], p["t"]
        mo = _rand(g, 2 * b, c, tt)
        mo[:b] *= (1.0 + torch.arange(b, dtype=torch.float32)).view(b, 1, 1)
        t["mo"] = mo
        d.update(b=b, c=c, t=tt, cfg_scale=p["scale"], phi=p["phi"])

    def _vae_sample(self, g, p, t, d):
        b, c, tt = p["b"], p["c"], p["t"]
        ms = _rand(g, b, 2 * c, tt) * 2.0
        ms[:, :c] += 3.0 * (1.0 + torch.arange(b, dtype=torch.float32)).view(b, 1, 1)            # means of about 3, 6, 9: never a scale
        planted = []
        if p["s"] == "all":
            for k, v in enumerate(VAE_PLANTED):
                pos = (k % b, (2 * k + 1) % c, (11 * k + 3) % tt)
                ms[pos[0], c + pos[1], pos[2]] = v
                planted.append((pos, v))
            ms[b - 1, 2 * c - 1, tt - 1] = 60.0
            planted.append(((b - 1, c - 1, tt - 1), 60.0))
            assert len({pos for pos, _ in planted}) == len(planted)
        else:
            ms[0, 1, 0] = p["s"]
            planted.append(((0, 0, 0), p["s"]))
        t["ms"], t["noise"] = ms, _rand(g, b, c, tt)
        d.update(b=b, c=c, t=tt, planted=planted)

    def _snake_beta(self, g, p, t, d):
        b, c, tt = p["b"], p["c"], p["t"]
        t["x"] = _rand(g, b, c, tt)            # |x exp(alpha)| stays within a few radians
        t["alpha"] = 0.2 * _rand(g, c)
        beta = p["beta"] + 0.3 * _rand(g, c)
        beta[0] = p["beta"]
        t["beta"] = beta
        d.update(b=b, c=c, t=tt)

    def _number_embed(self, g, p, t, d):
        half, feat = p["half"], p["features"]
        k = 2 * half + 1
        t["values"] = torch.tensor([-7.0, 0.0, 200.5, 512.0, 600.0]) if p["count"] == 5 else torch.tensor([200.5])
        t["w"] = 0.3 * _rand(g, half)            # |2 pi x w| stays within a few radians
        t["lw"], t["lb"] = _rand(g, feat, k) / math.sqrt(k), 0.3 * _rand(g, feat)
        d.update(count=p["count"], half=half, features=feat, min_val=0.0, max_val=512.0)

    def _float_to_int16(self, g, p, t, d):
        n, peak = p["n"], p["peak"]
        if p["where"] == "zero":
            x = torch.zeros(n)
        else:
            x = _rand(g, n)
            if p["where"] == "last":
                if n > 1:
                    x[:n - 1] *= 0.9 * peak / x[:n - 1].abs().max()
                x[n - 1] = -peak
            else:
                x *= peak / x.abs().max()
        t["x"] = x
        d.update(n=n, maximize=p["maximize"])

    def _overlap_add(self, g, p, t, d):
        b, n, c, l, hop, ov = (p[k] for k in ("batch", "chunks", "c", "l", "hop", "ov"))
        pieces = _rand(g, b, n, c, l) + 2.0
        pieces *= (1.0 + torch.arange(b * n * c, dtype=torch.float32)).view(b, n, c, 1) * 0.25            # every (item, chunk, channel) has its own level
        t["pieces"] = pieces
        t["window"] = torch.bartlett_window(max(ov, 1) * 2)
        d.update(batch=b, chunks=n, c=c, l=l, hop=hop, ov=ov, total=hop * (n - 1) + l + p["extra"])

    def _resample_sinc(self, g, p, t, d):
        from stable_audio_tools.inference.resample import sinc_resample_bank
        bank, width, orig, new = sinc_resample_bank(p["orig_sr"], p["new_sr"])
        rows, in_len = p["rows"], p["in_len"]
        t["bank"] = bank
        t["x"] = _rand(g, rows, in_len) * (1.0 + torch.arange(rows, dtype=torch.float32)).view(rows, 1)
        d.update(rows=rows, in_len=in_len, out_len=-(-in_len * new // orig) - p["short"], orig=orig, new=new, width=width)


# ----------------------------------------------------------------------------------------------------------------- the restatements
def overlap_add(pieces, window, hop, ov, total):
    """models/autoencoders.py:476-497 of the reference: chunk i, faded in over its first ``ov`` samples unless it is the first and out over its
    last ``ov`` unless it is the last, is added at i * hop.  pieces [batch, n_chunk, channels, L] -> [batch, channels, total]."""
    b, n, c, l = pieces.shape
    out = torch.zeros((b, c, total), dtype=pieces.dtype)
    for i in range(n):
        piece = pieces[:, i].clone()
        if ov and i != 0:
            piece[..., :ov] *= window[:ov]
        if ov and i != n - 1:
            piece[..., l - ov:] *= window[ov:2 * ov]
        lo, hi = i * hop, min(i * hop + l, total)
        if hi > lo:
            out[..., lo:hi] += piece[..., :hi - lo]
    return out


def resample_frames(x, bank, in_len, out_len, orig, new, width):
    """Output sample frame * new + phase is the dot product of row ``phase`` of the bank with the 2 * width + orig input samples that start at
    frame * orig - width, zeros outside the signal (torchaudio's _apply_sinc_resample_kernel: pad (width, width + orig), stride orig)."""
    taps = 2 * width + orig
    frames = -(-out_len // new)
    need = (frames - 1) * orig + taps
    pad = F.pad(x, (width, max(0, need - width - in_len)))
    win = pad.unfold(-1, taps, orig)[:, :frames]            # [rows, frames, taps]
    return torch.einsum("rft,pt->rfp", win, bank).reshape(x.shape[0], frames * new)[:, :out_len]


def softplus(x):
    """F.softplus with its defaults (beta 1, threshold 20): x above the threshold, log(1 + exp(x)) below."""
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def dpm_error_bound(n, n_partials):
    """Relative bound on |sum(partials) - reference| for ANY fp32 evaluation that gives each of n_partials workgroups of 256 threads a
    grid-strided share.  u = 2^-24.  Per term ((lo - hi) / max(atol, rtol max(|lo|, |prev|)))^2: |.| and max are exact; the subtraction and the
    product with rtol are one rounding each (u); the division is allowed 2.5 ulp = 5 u (1 u where it is correctly rounded); the quotient
    e therefore carries 7 u, its square 2 * 7 u + 1 u = 15 u.  Accumulation: a thread adds ceil(n / (256 n_partials)) terms in a chain, the wave
    reduction adds log2(64) = 6 levels, the four waves of the block 2 more, and every addition is one rounding on a partial sum that -- all
    terms being non-negative -- never exceeds the final one: chain + 8 roundings.  The float64 sum over the partials adds nothing at this
    scale.  1 % covers the second-order terms."""
    chain = -(-n // (256 * n_partials))
    return 1.01 * (15 + chain + 8) * UNIT


def _bound_terms(out, key, terms):
    """The magnitude sum |c| |t| over ``terms`` [(c, fp32 tensor)] and the number of products of the a-priori bound."""
    out[key + ":mag"], out[key + ":n"] = sum(abs(c) * x.to(F64).abs() for c, x in terms), len(terms)


def reference(case, dt=F64):
    k, t, d, p = case.kind, case.t, case.dim, case.p
    out = {}
    if k == "lincomb":
        terms = [(d["coef"][i], t[f"t{i}"]) for i in range(5) if t[f"t{i}"] is not None]
        if terms:
            out["out"] = sum(c * x.to(dt) for c, x in terms)
            _bound_terms(out, "out", terms)
        else:
            out["out"], out["out:mag"], out["out:n"] = torch.zeros(d["n"], dtype=dt), torch.zeros(d["n"], dtype=F64), 0
    elif k == "dpmpp3m_update":
        # x <- a x + b d + c1 (d - d1) + c2 (d1 - d2) + cn noise; a term whose tensor is NULL has a zero coefficient
        terms = [(d["a"], t["x"]), (d["b"], t["d"])]
        if d["c1"] != 0.0:
            terms += [(d["c1"], t["d"]), (-d["c1"], t["d1"])]
        if d["c2"] != 0.0:
            terms += [(d["c2"], t["d1"]), (-d["c2"], t["d2"])]
        if d["cn"] != 0.0:
            terms += [(d["cn"], t["noise"])]
        x, dd, d1, d2, nz = (_c(t[n], dt) for n in ("x", "d", "d1", "d2", "noise"))
        v = d["a"] * x + d["b"] * dd
        if d["c1"] != 0.0:
            v = v + d["c1"] * (dd - d1)
        if d["c2"] != 0.0:
            v = v + d["c2"] * (d1 - d2)
        if d["cn"] != 0.0:
            v = v + d["cn"] * nz
        out["x"] = v
        _bound_terms(out, "x", terms)
    elif k == "inpaint_mix":
        # get_bmask: torch.where(mask <= (i + 1) / steps, 1, 0) on the fp32 mask (the scalar takes the mask's dtype); x keeps init + noise sigma there
        keep = (t["mask"] <= torch.tensor(d["strength"], dtype=torch.float32)).view(1, -1).expand(d["rows"], d["t"])
        mixed = _c(t["init"], dt) + _c(t["noise"], dt) * d["sigma"]
        out["x"] = torch.where(keep, mixed, _c(t["x"], dt))
        out["x:mag"] = torch.where(keep, t["init"].to(F64).abs() + t["noise"].to(F64).abs() * abs(d["sigma"]), torch.zeros((), dtype=F64))
        out["x:n"] = 1
        out["x:keep"] = keep
    elif k == "dpm_error_partials":
        lo, hi, prev = (_c(t[n], dt) for n in ("x_low", "x_high", "x_prev"))
        delta = torch.clamp(d["rtol"] * torch.maximum(lo.abs(), prev.abs()), min=d["atol"])
        e2 = ((lo - hi) / delta).pow(2)
        # block-wise partial sums: workgroup j of n_partials takes every n_partials-th run of 256 elements
        per = 256 * d["parts"]
        e2 = F.pad(e2, (0, (-d["n"]) % per)).view(-1, d["parts"], 256)
        out["partial"] = e2.sum(dim=(0, 2))
    elif k == "cfg_combine":
        b = d["b"]
        cond, unc = _c(t["mo"], dt)[:b], _c(t["mo"], dt)[b:]
        v = unc + (cond - unc) * d["cfg_scale"]
        if d["phi"] != 0.0:
            v = v * (d["phi"] * (cond.std(dim=1, keepdim=True) / v.std(dim=1, keepdim=True)) + (1.0 - d["phi"]))
            out["out"] = v
        else:
            s = abs(d["cfg_scale"])
            out["out"], out["out:n"] = v, 2
            out["out:mag"] = t["mo"].to(F64)[b:].abs() * (1.0 + s) + t["mo"].to(F64)[:b].abs() * s
    elif k == "vae_sample":
        mean, scale = _c(t["ms"], dt).chunk(2, dim=1)
        out["z"] = _c(t["noise"], dt) * (softplus(scale) + 1e-4) + mean
    elif k == "snake_beta":
        x = _c(t["x"], dt)
        a, b = torch.exp(_c(t["alpha"], dt)).view(1, -1, 1), torch.exp(_c(t["beta"], dt)).view(1, -1, 1)
        out["y"] = x + torch.sin(x * a).pow(2) / (b + 1e-9)
    elif k == "number_embed":
        x = (_c(t["values"], dt).clamp(d["min_val"], d["max_val"]) - d["min_val"]) / (d["max_val"] - d["min_val"])
        f = x[:, None] * _c(t["w"], dt)[None, :] * 2.0 * math.pi
        feat = torch.cat((x[:, None], f.sin(), f.cos()), dim=-1)
        out["out"] = feat @ _c(t["lw"], dt).T + _c(t["lb"], dt)
    elif k == "float_to_int16":
        x = t["x"]
        if p["where"] == "zero":
            out["out"] = torch.zeros(d["n"], dtype=torch.int16)            # silence is silence under both settings
        else:
            div = x.abs().max().item()
            if not d["maximize"]:
                div = max(div, 1.0)
            out["out"] = x.div(div).mul(32767).to(torch.int16)
    elif k == "overlap_add":
        args = (d["hop"], d["ov"], d["total"])
        out["out"] = overlap_add(_c(t["pieces"], dt), _c(t["window"], dt), *args)
        out["out:mag"] = overlap_add(t["pieces"].to(F64).abs(), t["window"].to(F64).abs(), *args)
        out["out:n"] = overlap_add(torch.ones(t["pieces"].shape, dtype=F64), torch.ones(t["window"].shape, dtype=F64), *args)
    elif k == "resample_sinc":
        args = (d["in_len"], d["out_len"], d["orig"], d["new"], d["width"])
        out["y"] = resample_frames(_c(t["x"], dt), _c(t["bank"], dt), *args)
        out["y:mag"] = resample_frames(t["x"].to(F64).abs(), t["bank"].to(F64).abs(), *args)
        out["y:n"] = 2 * d["width"] + d["orig"]
    else:
        raise ValueError(k)
    return out


# ----------------------------------------------------------------------------------------------------------------------- the gates
def _index(flat, shape):
    return tuple(int(i) for i in torch.unravel_index(torch.tensor(int(flat)), shape)) if len(shape) else ()


def check(case, got, want=None, headroom=1.0):
    """Every output of ``got`` ({name: CPU tensor}) against ``want`` (reference(case) unless given) under the gates of the module docstring.
    Every failure names the kind, the case and the index."""
    want = reference(case) if want is None else want
    k, d = case.kind, case.dim
    tol = TOL * headroom
    for key, w in want.items():
        if ":" in key:
            continue
        g = got[key].detach().cpu()
        name = f"{case.name} {key}"
        assert tuple(g.shape) == tuple(w.shape), f"{name}: shape {tuple(g.shape)}, expected {tuple(w.shape)}"
        if k == "float_to_int16":
            assert g.dtype == torch.int16, f"{name}: dtype {g.dtype}"
            diff = (g != w).reshape(-1).nonzero()
            _note(case, key, "samples that differ", diff.shape[0])
            assert diff.shape[0] == 0, (f"{name}: {diff.shape[0]} of {w.numel()} samples differ from x.div(div).mul(32767).to(int16), the first at "
                                        f"{int(diff[0, 0])}: got {int(g.reshape(-1)[diff[0, 0]])}, want {int(w.reshape(-1)[diff[0, 0]])}")
            continue
        if k == "dpm_error_partials":
            gd = g.to(F64)
            bad = (~torch.isfinite(gd)).nonzero()
            assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} of {gd.numel()} partials were not written or are non-finite, the first at {int(bad[0, 0])}"
            neg = (gd < 0).nonzero()
            assert neg.shape[0] == 0, f"{name}: partial {int(neg[0, 0])} is negative ({gd[neg[0, 0]].item():.3e})"
            first_idle = -(-d["n"] // 256)
            idle = (gd[first_idle:] != 0.0).nonzero()
            assert idle.shape[0] == 0, (f"{name}: partial {first_idle + int(idle[0, 0])} belongs to a block without an element and holds "
                                        f"{gd[first_idle + int(idle[0, 0])].item():.3e} instead of 0.0")
            total, ref = gd.sum().item(), w.to(F64).sum().item()
            rel, bound = abs(total - ref) / ref, dpm_error_bound(d["n"], d["parts"])
            _note(case, key, "relative error of the sum", rel, f"bound {bound:.3e}")
            assert rel <= bound, f"{name}: sum of the partials {total!r} against {ref!r}: relative error {rel:.3e} > derived bound {bound:.3e} (index: the sum)"
            continue
        assert torch.isfinite(g.float()).all(), f"{name}: non-finite values, the first at {_index((~torch.isfinite(g.float())).reshape(-1).nonzero()[0, 0], g.shape)}"
        if key + ":mag" in want:
            share = bound_share(g, w, want[key + ":mag"], want[key + ":n"])
            worst = int(share.reshape(-1).argmax())
            _note(case, key, "largest share of the a-priori bound", share.reshape(-1)[worst].item(), str(_index(worst, share.shape)))
            bad = ~(share <= 1.0)
            assert not bool(bad.any()), (f"{name}: {int(bad.sum())} elements exceed the a-priori bound (n + 4) 2^-24 sum |c| |t|, the worst "
                                         f"{share.reshape(-1)[worst].item():.3g} x at {_index(worst, share.shape)}, the first at {tuple(int(i) for i in bad.nonzero()[0])}")
            if key + ":keep" in want:            # what the kernel leaves alone holds its input bit for bit
                keep = want[key + ":keep"]
                assert_bit_equal(f"{name} outside the kept region (flat index among the {int((~keep).sum())} untouched elements)",
                                 g[~keep], case.t[key][~keep])
            continue
        r = assert_close_sliced(name + " per element", g, w, tol, tuple(range(w.dim())))
        _note(case, key, "worst element", r[0], str(r[1]))
        if w.dim() > 1:
            rows = (0, 1) if w.dim() == 3 else (0,)
            r = assert_close_sliced(name + (" per (batch, channel) row" if w.dim() == 3 else " per row"), g, w, tol, rows)
            _note(case, key, "worst row", r[0], str(r[1]))
