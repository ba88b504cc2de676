"""Build extension: checks to run once on a checkpoint this build has never seen, before trusting its audio.

``check_fp16_range`` answers whether the package default -- IEEE fp16 operands, whose fp32 -> fp16 conversions saturate silently at
+-65504 -- is safe for a model: one generation with the range reports of the DiT (``DiffusionTransformer.activation_range_report``) and
of the codec (``AudioAutoencoder.activation_range_report``) switched on."""
import math

FP16_MAX = 65504.0
DIT_ADVICE = 'the DiT has activations at or beyond the fp16 range: model.model.model.set_gemm_dtype("bf16") (generate.py --gemm-dtype bf16)'
CODEC_ADVICE = ('the codec has activations at or beyond the fp16 range: model.pretransform.model.set_gemm_dtype("fp32") '
                "(generate.py --codec-dtype fp32)")


def summarize_fp16_range(dit_rows, codec_rows):
    """The verdict on the two tables (lists of dicts with at least ``max_abs``, ``over_fp16``, ``elements``): ``headroom`` = the smallest
    65504 / max_abs over every buffer that was written (``math.inf`` if all of them are zero), ``tightest`` = that row with a ``where`` key
    ("dit" / "codec"), ``advice`` = what to switch when ``over_fp16 > 0`` anywhere in the DiT (bf16 operands) or in the codec (the fp32
    build).  Changes nothing."""
    headroom, tightest = math.inf, None
    for where, rows in (("dit", dit_rows), ("codec", codec_rows)):
        for r in rows:
            if r["elements"] > 0 and r["max_abs"] > 0 and FP16_MAX / r["max_abs"] < headroom:
                headroom, tightest = FP16_MAX / r["max_abs"], dict(where=where, **r)
    advice = []
    if any(r["over_fp16"] > 0 for r in dit_rows):
        advice.append(DIT_ADVICE)
    if any(r["over_fp16"] > 0 for r in codec_rows):
        advice.append(CODEC_ADVICE)
    return dict(dit=list(dit_rows), codec=list(codec_rows), headroom=headroom, tightest=tightest, advice=advice)


def check_fp16_range(model, steps: int = 8, **generate_kwargs):
    """One ``generate_diffusion_cond(model, steps=steps, **generate_kwargs)`` with both range reports on; returns
    ``summarize_fp16_range`` of what they collected over ALL sampler steps and the decode (plus the encode of an init audio).  The
    reports are off again afterwards, also when the generation fails, and no setting of the model is changed: ``advice`` is for the
    caller to act on.  In an fp16 model ``over_fp16`` counts clamped values, so ``max_abs`` stops at 65504 there; run the check on a
    model set to bf16 (DiT) / fp32 (codec) to see how far beyond the range the activations go."""
    from .generation import generate_diffusion_cond
    dit = model.model.model
    codec = model.pretransform.model if model.pretransform is not None else None
    dit_rows, codec_rows = [], []
    dit.activation_range_report(True)
    try:
        if codec is not None:
            codec.activation_range_report(True)
        try:
            generate_diffusion_cond(model, steps=steps, **generate_kwargs)
        finally:
            if codec is not None:
                codec_rows = codec.activation_range_report(False)
    finally:
        dit_rows = dit.activation_range_report(False)
    return summarize_fp16_range(dit_rows, codec_rows)


def format_fp16_range(summary):
    """A few printable lines for ``generate.py --check-fp16-range``."""
    t = summary["tightest"]
    lines = [f"fp16 range check: {len(summary['dit'])} DiT buffers, {len(summary['codec'])} codec tensors"]
    if t is None:
        lines.append("  nothing was written")
    else:
        place = f"DiT layer {t['layer']} {t['buffer']}" if t["where"] == "dit" else f"codec {t.get('part', '')} {t['name']}".replace("  ", " ")
        lines.append(f"  smallest headroom 65504 / max|x| = {summary['headroom']:.3g} at {place} (max|x| = {t['max_abs']:.6g})")
    over = [("dit", r) for r in summary["dit"] if r["over_fp16"] > 0] + [("codec", r) for r in summary["codec"] if r["over_fp16"] > 0]
    for where, r in over[:8]:
        place = f"DiT layer {r['layer']} {r['buffer']}" if where == "dit" else f"codec {r.get('part', '')} {r['name']}".replace("  ", " ")
        lines.append(f"  {place}: {r['over_fp16']} of {r['elements']} elements at or beyond +-65504 ({r['nonfinite']} non-finite)")
    if len(over) > 8:
        lines.append(f"  ... and {len(over) - 8} more buffers")
    lines += [f"  advice: {a}" for a in summary["advice"]] or ["  no buffer reaches the fp16 range"]
    return lines
