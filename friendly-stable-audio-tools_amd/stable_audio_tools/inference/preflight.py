"""Build extension: checks to run once on a checkpoint this build has never seen, before trusting its audio.

``check_fp16_range`` answers whether the package default -- IEEE fp16 operands, whose fp32 -> fp16 conversions saturate silently at
+-65504 -- is safe for a model: one generation with the range reports of the DiT (``DiffusionTransformer.activation_range_report``) and
of the codec (``AudioAutoencoder.activation_range_report``) switched on."""
import math

FP16_MAX = 65504.0
DIT_ADVICE = ("the DiT has fp16 blocks with activations at or beyond the fp16 range: run those blocks in bf16 -- preflight.apply_fp16_range_fix(model, ...) "
              "or model.model.model.set_block_gemm_dtypes(preflight.choose_block_formats(summary)) (generate.py --gemm-dtype auto)")
CODEC_ADVICE = ('the codec has activations at or beyond the fp16 range: model.pretransform.model.set_gemm_dtype("fp32") '
                "(generate.py --codec-dtype fp32)")


def summarize_fp16_range(dit_rows, codec_rows):
    """The verdict on the two tables (lists of dicts with at least ``max_abs``, ``over_fp16``, ``elements``): ``headroom`` = the smallest
    65504 / max_abs over every buffer that was written (``math.inf`` if all of them are zero), ``tightest`` = that row with a ``where`` key
    ("dit" / "codec"), ``advice`` = what to switch when ``over_fp16 > 0`` anywhere in the DiT (bf16 operands for those blocks) or in the
    codec (the fp32 build).  A DiT row whose ``format`` is "bf16" (a block ``set_block_gemm_dtypes`` already runs in bf16) is handled: its
    ``over_fp16`` counts what fp16 WOULD clamp, nothing was, and neither the advice nor the headroom looks at it; ``handled`` counts those
    rows with ``over_fp16 > 0``.  Changes nothing."""
    headroom, tightest = math.inf, None
    for where, rows in (("dit", dit_rows), ("codec", codec_rows)):
        for r in rows:
            if r.get("format") == "bf16":
                continue
            if r["elements"] > 0 and r["max_abs"] > 0 and FP16_MAX / r["max_abs"] < headroom:
                headroom, tightest = FP16_MAX / r["max_abs"], dict(where=where, **r)
    advice = []
    if any(r["over_fp16"] > 0 and r.get("format") != "bf16" for r in dit_rows):
        advice.append(DIT_ADVICE)
    if any(r["over_fp16"] > 0 for r in codec_rows):
        advice.append(CODEC_ADVICE)
    handled = sum(1 for r in dit_rows if r["over_fp16"] > 0 and r.get("format") == "bf16")
    return dict(dit=list(dit_rows), codec=list(codec_rows), headroom=headroom, tightest=tightest, advice=advice, handled=handled)


def choose_block_formats(summary, min_headroom: float = 1.0):
    """The operand format per DiT block that ``summary`` (``summarize_fp16_range`` / ``check_fp16_range``) asks for, as
    ``DiffusionTransformer.set_block_gemm_dtypes`` takes it: "bf16" for every layer with a DiT row where ``over_fp16 > 0`` or
    ``max_abs * min_headroom >= 65504`` (``min_headroom`` 2.0 also moves blocks that use more than half the range), "fp16" for the others.
    One entry per layer 0 .. the largest ``layer`` among the rows.  Pure Python, changes nothing."""
    rows = summary["dit"]
    depth = max((r["layer"] for r in rows), default=-1) + 1
    formats = ["fp16"] * depth
    for r in rows:
        if r["over_fp16"] > 0 or (r["elements"] > 0 and r["max_abs"] * min_headroom >= FP16_MAX):
            formats[r["layer"]] = "bf16"
    return formats


def apply_fp16_range_fix(model, min_headroom: float = 1.0, steps: int = 8, **generate_kwargs):
    """``check_fp16_range``, then ``set_block_gemm_dtypes(choose_block_formats(...))`` on the DiT, then the check once more on the model as it
    now runs; returns ``(before, after)``, the two summaries.  The DiT's ``gemm_dtype`` must be "fp16" or "bf16" (``NotImplementedError``
    otherwise); blocks an earlier call already moved to bf16 stay there as long as their rows still ask for it.  Afterwards no fp16 block of
    the DiT should have a clamped value over this generation: ``after["advice"]`` says so if one still has (un-clamping a block can push a
    later one over; call again then).  The codec is only reported on."""
    dit = model.model.model
    before = check_fp16_range(model, steps=steps, **generate_kwargs)
    dit.set_block_gemm_dtypes(choose_block_formats(before, min_headroom))
    after = check_fp16_range(model, steps=steps, **generate_kwargs)
    return before, after


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
    bf16_blocks = sorted({r["layer"] for r in summary["dit"] if r.get("format") == "bf16" and r["over_fp16"] > 0})
    if bf16_blocks:
        lines.append(f"  DiT blocks {bf16_blocks} run in bf16: their values beyond +-65504 are kept, not clamped")
    over = ([("dit", r) for r in summary["dit"] if r["over_fp16"] > 0 and r.get("format") != "bf16"] +
            [("codec", r) for r in summary["codec"] if r["over_fp16"] > 0])
    for where, r in over[:8]:
        place = f"DiT layer {r['layer']} {r['buffer']}" if where == "dit" else f"codec {r.get('part', '')} {r['name']}".replace("  ", " ")
        lines.append(f"  {place}: {r['over_fp16']} of {r['elements']} elements at or beyond +-65504 ({r['nonfinite']} non-finite)")
    if len(over) > 8:
        lines.append(f"  ... and {len(over) - 8} more buffers")
    lines += [f"  advice: {a}" for a in summary["advice"]] or ["  no buffer reaches the fp16 range"]
    return lines
