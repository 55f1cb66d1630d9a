#!/usr/bin/env python3
"""What the frame dedup costs a scene that has nothing to deduplicate.

bench.py's headline scene (N anchors, the same N images again as queries) with the query half
replaced by N other seeded images, so Aggregator._embed pays the fingerprint pass, the candidate /
compare / output launches and the one read-back, and then runs the DINO stack on every frame as
with SR_DEDUP_FRAMES=0.  One process, one model; the two arms alternate (off, on, off, on, ...),
each round timing --steps forwards between device synchronisations.  Prints one JSON line.

    python tools/bench_distinct.py --views 32 --steps 10 --rounds 3
    python tools/bench_distinct.py --duplicated      # the headline scene itself, same protocol
"""

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--img", type=int, default=518)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--duplicated", action="store_true", help="queries = the anchor images (bench.py's scene)")
    args = ap.parse_args()

    import bench
    from sailrecon_amd.models import aggregator as A

    device = torch.device("cuda", 0)
    model, _ = bench.build_model(device)
    n = args.views
    x = torch.rand(n, 3, args.img, args.img, generator=torch.Generator().manual_seed(n))
    q = x if args.duplicated else torch.rand(n, 3, args.img, args.img, generator=torch.Generator().manual_seed(n + 1000))
    images = torch.cat([x, q])[None].to(device)
    no_reloc, reloc = list(range(n)), list(range(n, 2 * n))

    def step():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model(images, no_reloc_list=no_reloc, reloc_list=reloc, fix_rank=300)

    ms = {"off": [], "on": []}
    groups = {}
    for arm in ("off", "on"):
        A._DEDUP_FRAMES = arm == "on"
        for _ in range(args.warmup):
            step()
        groups[arm] = model.aggregator.last_frame_groups
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for arm in ("off", "on"):
            A._DEDUP_FRAMES = arm == "on"
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) / args.steps * 1e3)
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    print(json.dumps({"scene": "duplicated" if args.duplicated else "distinct", "views": n, "img": args.img,
                      "steps": args.steps, "rounds": args.rounds, "frame_groups": groups,
                      "step_ms": {k: [round(t, 3) for t in v] for k, v in ms.items()},
                      "mean_ms": {k: round(v, 3) for k, v in mean.items()},
                      "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "on_minus_off_ms": round(mean["on"] - mean["off"], 3)}))


if __name__ == "__main__":
    main()
