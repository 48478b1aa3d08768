"""Step times of paper mode (dvcp.paper.DeepVCPPaper): train_extractor, train_heads and inference
steps alternating in one process (DESIGN.md 4.6's recipe: one pair of 16384 points, K = 64, r = 2.0,
s = 0.4, 3 warm-up and 10 timed steps, a host clock around a device synchronise), peak allocated
memory per kind of step and, with --events, the per-entry HIP-event times of one step of the first
kind.  One JSON line on stdout.

  python tools/paper_step_bench.py --tag change --events
  python tools/paper_step_bench.py --root <another checkout, built> --kinds heads,infer --tag parent

Kind ``bnheads``: a head-training step after ``model.train(); model.FE.eval()`` on a model built with
``bn_train=True`` (batch-statistics BN in both weighting layers over a frozen-BN extractor); every
other kind runs in eval mode.  Kind ``bntrain``: the whole network in training mode (``model.train()``,
``train_extractor``, every parameter trainable): batch statistics in the extractor and the heads.

--root: the tree whose package is measured (default: this one), for A/B runs in alternating
processes; a tree without train_extractor takes --kinds heads,infer.  --out: also write the JSON there."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--kinds", default="extractor,heads,infer")
ap.add_argument("--tag", default="run")
ap.add_argument("--out", default=None)
ap.add_argument("--events", action="store_true")
args = ap.parse_args()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, "deepvcp-pointcloud-registration_amd"))

import torch  # noqa: E402

import dvcp  # noqa: E402
from dvcp import _lib  # noqa: E402
from dvcp.synthetic import make_pairs  # noqa: E402

dev = torch.device("cuda:0")
kinds = args.kinds.split(",")
src, tgt, R, t = make_pairs(1, 16384, seed=5)
src, tgt, R, t = src.float().to(dev), tgt.float().to(dev), R.to(dev), t.to(dev)
torch.manual_seed(0)
flags = {"bn_train": True} if ("bnheads" in kinds or "bntrain" in kinds) else {}   # a tree without the flag is never asked for the kind
model = dvcp.paper.DeepVCPPaper(use_normal=False, K=64, r=2.0, s=0.4, s_z=0.25, **flags).eval().to(dev)
starts = torch.stack([model.FE.draw_starts(1, 16384), model.FE.draw_starts(1, 16384)])
opt = torch.optim.Adam(model.parameters(), lr=1e-5)
t0 = torch.zeros(1, 3)


def step(kind):
    model.eval()
    if kind == "bnheads":
        model.train()
        model.FE.eval()
    if kind == "bntrain":
        model.train()
    if kind == "infer":
        with torch.no_grad():
            return model(src, tgt, R, t0, starts=starts)
    model.train_heads = kind in ("heads", "bnheads")
    model.train_extractor = kind in ("extractor", "bntrain")
    model.FE.requires_grad_(kind in ("extractor", "bntrain"))
    opt.zero_grad(set_to_none=True)
    out = model(src, tgt, R, t0, starts=starts)
    loss = 0.0
    for st in out:
        loss = loss + dvcp.paper.deepVCP_loss_paper(st["keypts"], st["vcp"], st["weights"], R, t, 0.5, inlier_ratio=0.8)[0]
    loss.backward()
    opt.step()
    return loss


times = {k: [] for k in kinds}
peak = {k: 0 for k in kinds}
for i in range(13):
    for k in kinds:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        a = time.perf_counter()
        step(k)
        torch.cuda.synchronize()
        b = time.perf_counter()
        if i >= 3:
            times[k].append((b - a) * 1e3)
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
res = {"tag": args.tag, "device": torch.cuda.get_device_name(0)}
for k in kinds:
    res[k] = {"median_ms": round(statistics.median(times[k]), 3), "min_ms": round(min(times[k]), 3),
              "max_ms": round(max(times[k]), 3), "peak_MiB": round(peak[k] / 2 ** 20, 1)}
if args.events:
    _lib.EVENT_LOG = []
    step(kinds[0])
    torch.cuda.synchronize()
    per = {}
    for name, e0, e1, _ in _lib.EVENT_LOG:
        n, ms = per.get(name, (0, 0.0))
        per[name] = (n + 1, ms + e0.elapsed_time(e1))
    _lib.EVENT_LOG = None
    res["events_" + kinds[0]] = {k: {"calls": n, "ms": round(ms, 4)} for k, (n, ms) in sorted(per.items(), key=lambda kv: -kv[1][1])}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
