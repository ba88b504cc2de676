"""The single-kernel cases of the patchified DiT's boundary kernels (csrc/dit_patch.hip): shapes, seeded inputs, a restatement of every
operation in plain PyTorch, and the faults the gates have to reject.  The device test (test_gpu_dit_patch_kernels.py) runs each kernel
through its unit entry and compares with ``reference(case)`` in float64 under the gates of fp32_units.check (elementwise under
(n + 4) 2^-24 |W| |x| with n the contraction length, 1e-5 per row and 32 x 32 block); the host test (test_dit_patch_host.py) proves these
references against plain fp32 PyTorch -- reshape / permute, 1x1 conv, Linear -- and shows that the gates reject the faults of ``FAULTS``.

``patchify`` / ``unpatchify`` restate the reference's two rearranges (models/dit.py:207,222); tests/golden/make_golden_dit_families.py checks them
against einops on the golden cases' shapes."""
import torch
import torch.nn.functional as F

import fp32_units as fu


def patchify(x, P):
    """'b (t p) c -> b t (c p)'"""
    b, T, c = x.shape
    return x.reshape(b, T // P, P, c).permute(0, 1, 3, 2).reshape(b, T // P, c * P)


def unpatchify(o, P):
    """'b (c p) t -> b c (t p)'"""
    b, cp, t = o.shape
    return o.reshape(b, cp // P, P, t).permute(0, 1, 3, 2).reshape(b, cp // P, t * P)


# (Bf, C, Cc, P, T, D, p_len) + what is not the default (tc: concat length, xb: latents under the Bf sequences, xscale)
SHAPES = [
    dict(bf=1, c=4, cc=0, P=2, t=2, d=128, pl=0),                     # a single token
    dict(bf=3, c=64, cc=0, P=2, t=18, d=256, pl=0),                   # 9 tokens: a tail in IP_TT and OP_TOK, tokens of two sequences in one output workgroup
    dict(bf=2, c=64, cc=0, P=4, t=76, d=384, pl=0),                   # D no multiple of 256, four column groups
    dict(bf=2, c=8, cc=0, P=8, t=72, d=128, pl=0),
    dict(bf=2, c=64, cc=0, P=3, t=63, d=256, pl=0),                   # channels whose three columns straddle two column groups
    dict(bf=2, c=64, cc=8, P=2, t=78, d=256, pl=3, tc=26),            # resize, prepend copy
    dict(bf=2, c=64, cc=8, P=2, t=78, d=256, pl=3, tc=78),            # no resize
    dict(bf=4, c=64, cc=0, P=2, t=16, d=256, pl=0, xb=2),             # the CFG halves share x
    dict(bf=2, c=64, cc=0, P=2, t=16, d=256, pl=0, xscale=0.37),
]


def shape_id(p):
    return "-".join(f"{k}{v}" for k, v in p.items())


class Case:
    """kind in ("fold_in", "fold_out", "input_proj", "output_proj") + a shape of SHAPES -> seeded fp32 inputs ``t`` and dimensions ``dim``.
    ``kind`` is also what fp32_units.check reads: the contraction gates and the row view of fp32_units' case of that name."""

    def __init__(self, kind, p):
        self.p = dict(p)
        self.kind = "input_proj_extra" if kind == "input_proj" and (p["cc"] or p["pl"]) else kind
        self.what = kind
        self.name = f"{kind}_patch {shape_id(p)}"
        g = fu._gen(kind + "_patch", p)
        bf, c, cc, P, T, D, pl = (p[k] for k in ("bf", "c", "cc", "P", "t", "d", "pl"))
        xb, ci, tt = p.get("xb", bf), c + cc, T // P
        s = tt + (pl + 1 if pl or cc else 0)            # the extra-conditioning shapes stand for a "prepend" plan: prepend rows + global token
        t = self.t = {}
        # the raw weights, and the folded images as float64 rounds them: what each kernel is GIVEN (the folds have cases of their own)
        t["w_in"], t["w_pre"] = fu._rand(g, D, ci * P) * 0.3, fu._rand(g, ci, ci) * 0.3
        t["w_out"], t["w_post"] = fu._rand(g, c * P, D) * 0.2, fu._rand(g, c, c) * 0.3
        t["weff_in_t"] = fold_in(t["w_in"].double(), t["w_pre"].double(), P).float()
        t["weff_out_t"] = fold_out(t["w_out"].double(), t["w_post"].double(), P).float()
        t["x"] = fu._rand(g, xb, c, T)
        if xb > 1:
            t["x"][1] *= 8.0            # b % xB: the second latent is 8 x the first
        t["concat"] = fu._rand(g, bf, cc, p["tc"]) * (1.0 + torch.arange(bf, dtype=torch.float32)[:, None, None]) if cc else None
        t["prep"] = fu._rand(g, bf, pl, D) if pl else None
        X = fu._rand(g, bf, s, D)
        if bf > 1:
            X[1] *= 8.0            # a token row taken from the neighbouring sequence dominates
        t["X"] = X
        self.dim = dict(bf=bf, xb=xb, c=c, cc=cc, P=P, t=T, tt=tt, s=s, d=D, pl=pl, tc=p.get("tc", 0),
                        xscale=float(torch.tensor(p.get("xscale", 1.0), dtype=torch.float32)))


def fold_in(w_in, w_pre, P):
    """(project_in o patchify o (I + preprocess_conv))^T: [Ci P, D], Weff[n, c' P + p] = sum_c W_in[n, c P + p] (I + W_pre)[c, c']"""
    d, k = w_in.shape
    ci = k // P
    return torch.einsum("ncp,ce->nep", w_in.reshape(d, ci, P), torch.eye(ci, dtype=w_in.dtype) + w_pre).reshape(d, k).T.contiguous()


def fold_out(w_out, w_post, P):
    """((I + postprocess_conv) o unpatchify o project_out)^T: [D, C P], Weff[c' P + p, :] = sum_c (I + W_post)[c', c] W_out[c P + p, :]"""
    n, d = w_out.shape
    c = n // P
    return torch.einsum("ec,cpn->epn", torch.eye(c, dtype=w_out.dtype) + w_post, w_out.reshape(c, P, d)).reshape(n, d).T.contiguous()


FAULTS = ("in_pc", "out_pc", "frame_off_by_one", "prepend_off_by_one", "concat_src_per_token", "xscale_on_concat")


def _pc(x, P):
    """patchify with the feature index p C + c: 'b (t p) c -> b t (p c)'"""
    b, T, c = x.shape
    return x.reshape(b, T // P, P * c)


def reference(case, dt=torch.float64, fault=None):
    """{output: tensor} (+ ":mag" / ":n" of the a-priori bound) of the case's kernel on its fp32 inputs, evaluated in ``dt``.  ``fault``: the
    same with one of FAULTS built in (what a kernel with that mistake returns)."""
    t, d, f64 = case.t, case.dim, torch.float64
    c_ = lambda x: None if x is None else x.to(dt)
    P, c, cc = d["P"], d["c"], d["cc"]
    out = {}
    if case.what == "fold_in":
        ci = c + cc
        eye_abs = torch.eye(ci, dtype=f64) + t["w_pre"].to(f64).abs()
        mag = torch.einsum("ncp,ce->nep", t["w_in"].to(f64).abs().reshape(d["d"], ci, P), eye_abs).reshape(d["d"], ci * P).T.contiguous()
        fu._contract(out, "weff_t", fold_in(c_(t["w_in"]), c_(t["w_pre"]), P), mag, ci + 1)
    elif case.what == "fold_out":
        eye_abs = torch.eye(c, dtype=f64) + t["w_post"].to(f64).abs()
        mag = torch.einsum("ec,cpn->epn", eye_abs, t["w_out"].to(f64).abs().reshape(c, P, d["d"])).reshape(c * P, d["d"]).T.contiguous()
        fu._contract(out, "weff_t", fold_out(c_(t["w_out"]), c_(t["w_post"]), P), mag, c + 1)
    elif case.what == "input_proj":
        item = torch.arange(d["bf"]) % d["xb"]
        pat = _pc if fault == "in_pc" else patchify

        def frames(sig):            # [bf, ch, T] -> tokens [bf, T', ch P]
            if fault == "frame_off_by_one":            # frame t' P + p + 1 where t' P + p belongs (the last one clamped)
                sig = sig[:, :, (torch.arange(d["t"]) + 1).clamp_max(d["t"] - 1)]
            return pat(sig.transpose(1, 2), P)

        def term(w, sig, scale):
            return (frames(c_(sig)) @ c_(w)) * scale, (frames(sig.to(f64).abs()) @ w.to(f64).abs()) * scale

        w = t["weff_in_t"]
        v, mag = term(w[:c * P], t["x"][item], d["xscale"])
        if cc:
            if fault == "concat_src_per_token":            # one source frame per token, that of its first frame
                src = fu.nearest_src(d["tc"], d["t"])[(torch.arange(d["t"]) // P) * P]
            else:
                src = fu.nearest_src(d["tc"], d["t"])
            v2, mag2 = term(w[c * P:], t["concat"][:, :, src], d["xscale"] if fault == "xscale_on_concat" else 1.0)
            v, mag = v + v2, mag + mag2
        if fault == "prepend_off_by_one":            # the token rows one row late: row off + t' holds token t' - 1
            v = torch.roll(v, 1, dims=1)
        if t["prep"] is not None:
            out["prep"] = t["prep"]
        fu._contract(out, "X", v, mag, (c + cc) * P + 1)            # (+ 1: the multiplication by xscale)
    elif case.what == "output_proj":
        X = t["X"][:, d["s"] - d["tt"]:]
        un = (lambda o, P: o.reshape(o.shape[0], P, o.shape[1] // P, o.shape[2]).permute(0, 2, 3, 1).reshape(o.shape[0], o.shape[1] // P, -1)) \
            if fault == "out_pc" else unpatchify
        if fault == "frame_off_by_one":
            un = lambda o, P: torch.roll(unpatchify(o, P), 1, dims=2)
        if fault == "prepend_off_by_one":
            X = t["X"][:, d["s"] - d["tt"] - 1:-1]
        w = t["weff_out_t"]
        fu._contract(out, "out", un((c_(X) @ c_(w)).transpose(1, 2), P), un((X.to(f64).abs() @ w.to(f64).abs()).transpose(1, 2), P), d["d"])
    else:
        raise ValueError(case.what)
    return out


# ---- the same in plain fp32 PyTorch from the RAW weights, module by module as the reference model runs them (dit.py:167-173,197-224)
def torch_input(case, dt=torch.float32):
    t, d = case.t, case.dim
    x = t["x"].to(dt)[torch.arange(d["bf"]) % d["xb"]] * d["xscale"]            # VDenoiser scales the latent, the concat signal travels in the kwargs
    if d["cc"]:
        x = torch.cat([x, F.interpolate(t["concat"].to(dt), (d["t"],), mode="nearest")], dim=1)
    x = x + F.conv1d(x, t["w_pre"].to(dt)[:, :, None])
    return F.linear(patchify(x.transpose(1, 2), d["P"]), t["w_in"].to(dt))            # [bf, T', D]: the rows behind the prepended ones


def torch_output(case, dt=torch.float32):
    t, d = case.t, case.dim
    o = F.linear(t["X"].to(dt), t["w_out"].to(dt)).transpose(1, 2)[:, :, d["s"] - d["tt"]:]
    o = unpatchify(o, d["P"])
    return o + F.conv1d(o, t["w_post"].to(dt)[:, :, None])
