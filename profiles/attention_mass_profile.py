"""The attention-mass measurement points of DESIGN.md section 11f, one per process so that each can sit under
`rocprofv3 --kernel-trace --stats` in a run of its own (no counters):

    python profiles/attention_mass_profile.py c2_one       # 16 x 4096 / 4096, C2 flow, one layer's mass
    python profiles/attention_mass_profile.py c2_all       # the same batch, layers="all" (116 attentions)
    python profiles/attention_mass_profile.py native       # 20 x 1024 / 1250, C4 flow, layers aug / 50 / 110
    python profiles/attention_mass_profile.py weights_c2   # the full [16, 4096, 4096] map of one layer (attn_weights_kernel), for comparison
    python profiles/attention_mass_profile.py summarize DIR OUT.csv   # per-kernel median / mean / min / max of the traces under DIR

Module-initialised weights (kernel times do not depend on the values), 1 warm-up call and 3 calls per point."""
import contextlib
import csv
import glob
import io
import os
import statistics
import sys

REPEATS = 3


def _model(name, device, **kw):
    import torch
    import flowcompare_amd as fa
    cfg = fa.named_config(name, **kw)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        md = fa.initialize_flow(cfg, device=device, mode="test")
    return cfg, md


def run(point, device="cuda:0"):
    import torch
    import flowcompare_amd as fa
    g = torch.Generator().manual_seed(1)
    if point == "native":
        B, N, M = 20, 1024, 1250
        cfg, md = _model("c4_dgcnn_attn_extra_affine", device, sample_size=N)
        extra = (torch.rand(B, 1, generator=g) * 15).to(device)
        call = lambda: fa.attention_mass(batch, md, cfg, layers=("aug", 50, 110), weights=w, eps=eps)
    else:
        B, N, M = 16, 4096, 4096
        cfg, md = _model("c2_dgcnn_attn_spline", device, sample_size=N, **({"n_flow_layers": 2} if point == "weights_c2" else {}))
        extra = None
        if point == "weights_c2":
            call = lambda: fa.attention_weights(batch, md, cfg, layers=(1,), eps=eps)
        else:
            call = lambda: fa.attention_mass(batch, md, cfg, layers="all" if point == "c2_all" else (50,), weights=w, eps=eps)
    batch = (torch.rand(B, M, 6, generator=g).to(device), torch.rand(B, N, 6, generator=g).to(device), extra)
    eps = [torch.randn(s, generator=g).to(device) for s in md["flow"].noise_shapes(B, N)]
    w = torch.rand(B, N, generator=g).to(device)
    for _ in range(1 + REPEATS):
        out = call()
        torch.cuda.synchronize()
        del out
    print(f"{point}: B {B} N {N} M {M}, {1 + REPEATS} calls done")


def summarize(root, out_csv):
    """root/<point>/**/*kernel_trace.csv -> one row per (point, kernel whose name holds 'attn'): calls, median, mean, min, max in ns"""
    rows = []
    for point in sorted(os.listdir(root)):
        durations = {}
        for path in glob.glob(os.path.join(root, point, "**", "*kernel_trace.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    if "attn" in r["Kernel_Name"]:
                        durations.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        for name, d in sorted(durations.items()):
            rows.append([point, name, len(d), int(statistics.median(d)), round(statistics.fmean(d), 1), min(d), max(d)])
    with open(out_csv, "w", newline="") as f:
        wr = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
        wr.writerow(["point", "Name", "Calls", "MedianNs", "AverageNs", "MinNs", "MaxNs"])
        wr.writerows(rows)
    for r in rows:
        print(r)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1])
