"""Per-launch share of the f32 MFMA peak for tools/codec_only.py fp32 under rocprofv3 --kernel-trace: usage
   python tools/codec_fp32_share.py <pid>_kernel_trace.csv
Matches the last traced decode (38 launches) and encode (37) against the SA VAE layer list and prints useful FLOP / kernel time per layer."""
import csv
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1]))]
convs = [r for r in rows if "conv_pipe_kernel" in r["Kernel_Name"] or "first_conv_kernel" in r["Kernel_Name"] or "cf_to_cl" in r["Kernel_Name"]]
PEAK = 157.3e12
ch, cm, st, T = 128, [1, 2, 4, 8, 16], [2, 4, 4, 8, 8], 1024
def dec_layers():
    out = [("cf_to_cl", 0)]
    L = T; ctop = cm[-1] * ch
    out.append(("dec first k7 64->2048", 2 * L * ctop * 7 * 64))
    nb = 5
    for bi in range(nb):
        i = nb - bi
        cin = cm[i - 1] * ch; cout = (cm[i - 2] if i - 2 >= 0 else 1) * ch; s = st[i - 1]
        out.append((f"convT s{s} {cin}->{cout}", 2 * L * s * cout * 2 * cin))      # useful: output samples x cout x (2 taps x cin)... each output uses 2 taps
        L *= s
        for r in range(3):
            out.append((f"ru k7 C{cout} L{L}", 2 * L * cout * 7 * cout))
            out.append((f"ru k1 C{cout}", 2 * L * cout * cout))
    out.append(("final k7 128->2", 2 * L * 2 * 7 * 128))
    return out
def enc_layers():
    out = [("first_conv", 2 * T * 2048 * 128 * 14)]
    L = T * 2048
    for bi in range(5):
        cin = (1 if bi == 0 else cm[bi - 1]) * ch; cout = cm[bi] * ch; s = st[bi]
        for r in range(3):
            out.append((f"ru k7 C{cin} L{L}", 2 * L * cin * 7 * cin))
            out.append((f"ru k1 C{cin}", 2 * L * cin * cin))
        L //= s
        out.append((f"strided s{s} {cin}->{cout}", 2 * L * cout * 2 * s * cin))
    out.append(("final k3 2048->128", 2 * L * 128 * 3 * 2048))
    return out
def report(name, layers, seq):
    tot_t = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in seq)
    tot_f = sum(f for _, f in layers)
    print(f"\n== {name}: {len(seq)} launches, kernel time {tot_t/1e6:.2f} ms, useful {tot_f/1e12:.3f} TFLOP -> {tot_f/tot_t*1e-3:.1f} TF/s = {tot_f/tot_t*1e9/PEAK:.2f} of the f32 peak")
    agg = {}
    for (lname, f), r in zip(layers, seq):
        t = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        kn = r["Kernel_Name"].split("(")[0].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "")
        print(f"  {lname:28s} {kn:40s} {t/1e3:9.1f} us  {f/1e9:8.1f} GFLOP  {f/t*1e-3 if t else 0:6.1f} TF/s  {f/t*1e9/PEAK if t else 0:5.2f} of peak")
# last decode and last encode of the timed loops: decode launches = 2 + 5*7 + 1 = 38, encode = 1 + 5*7 + 1 = 37
dl, el = dec_layers(), enc_layers()
assert len(dl) == 38 and len(el) == 37
# sequence: [warm dec, 5 dec, warm enc, 5 enc] with vae_sample / randn in between encodes: pick by pattern
i = 0; runs = []
while i < len(convs):
    if "cf_to_cl" in convs[i]["Kernel_Name"]:
        runs.append(("dec", convs[i:i + 38])); i += 38
    elif "first_conv" in convs[i]["Kernel_Name"]:
        runs.append(("enc", convs[i:i + 37])); i += 37
    else:
        i += 1
decs = [s for k, s in runs if k == "dec"]; encs = [s for k, s in runs if k == "enc"]
print(f"{len(decs)} decodes, {len(encs)} encodes traced (under rocprofv3)")
report("decode 1024 frames (last traced)", dl, decs[-1])
report("encode 2097152 samples (last traced)", el, encs[-1])
