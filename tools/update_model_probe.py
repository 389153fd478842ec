#!/usr/bin/env python3
"""Where a keyframe's update_model spends its time outside the iterations, on a C4-sized local model (150 k surfels,
128x1024, window of 8).

    python tools/update_model_probe.py [--draw torch|device]
        cProfile of the HOST time of four updates (the iterations are cut to ITERS=2 so that the cold stages dominate)
    python tools/update_model_probe.py --ab [--blocks B] [--iters N] [--out FILE.json]
        A/B of the densify draw in ONE process: blocks that alternate draw="torch" (torch.multinomial) and
        draw="device" (the seeded sls_densify_draw) on the same keyframes, each block on a fresh copy of the model;
        update_model(timings=True) gives the stages (device synchronised between them); medians over the blocks
    python tools/update_model_probe.py --draws-only N
        N device draws and N torch draws (+ the mask's nonzero()) on one keyframe as a model's FIRST keyframe (every valid
        pixel a candidate) and nothing else (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import cProfile
import json
import os
import pstats
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from splat_loam_amd import fused_mapper, synth
from splat_loam_amd.renderer import depth_to_points
from splat_loam_amd.scene import Camera, SurfelModel

ap = argparse.ArgumentParser()
ap.add_argument("--draw", choices=("torch", "device"), default="torch")
ap.add_argument("--ab", action="store_true")
ap.add_argument("--blocks", type=int, default=6)
ap.add_argument("--iters", type=int, default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--draws-only", type=int, default=0)
args = ap.parse_args()

dev = "cuda:0"
n0, H, W, n_kf = 150_000, 128, 1024, 8
sc = synth.make_scene(n0, H, W, seed=0)
d, v = synth.make_targets(H, W, sc)
poses = synth.keyframe_poses(n_kf + 6)


def frame(k):
    cam = Camera(sc["K"], d, None, v, poses[k], data_device=dev)
    pts = depth_to_points(cam, cam.image_depth)
    cam.image_normal = (-pts / pts.norm(dim=0, keepdim=True).clamp_min(1e-9)).contiguous()
    return SimpleNamespace(camera=cam, model_T_frame=torch.tensor(poses[k], dtype=torch.float32, device=dev))


iters = args.iters if args.iters is not None else int(os.environ.get("ITERS", "200" if args.ab else "2"))
mapping = SimpleNamespace(num_iterations=iters, densify_threshold_egeom=-1.0, densify_threshold_opacity=0.5,
                          densify_percentage=0.15, prob_view_last_keyframe=0.4, pruning_min_opacity=0.0, pruning_min_size=0.0,
                          opt_lambda_alpha=0.1, opt_lambda_normal=0.1, opt_scaling_max=0.5, opt_scaling_max_penalty=0.2)
cfg = SimpleNamespace(mapping=mapping, opt=SimpleNamespace(depth_ratio=0.0))
frames = [frame(k) for k in range(n_kf + 6)]


def fresh_model():
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=dev)
    model.training_setup(fused=True)
    return model


def update(model, kfs, k, draw, gen, timings=False):
    if draw == "device":
        return fused_mapper.update_model(model, kfs, frames[k], cfg, draw="device", seed=0, timings=timings)
    return fused_mapper.update_model(model, kfs, frames[k], cfg, generator=gen, timings=timings)


def block(draw, updates=4):
    """A fresh model, two un-timed updates (allocator, the engine, first launches), then `updates` timed ones."""
    model, kfs = fresh_model(), frames[:n_kf]
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    np.random.seed(0)
    rows = []
    for j, k in enumerate(range(n_kf, n_kf + 2 + updates)):
        kfs = kfs[1:] + [frames[k]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = update(model, kfs, k, draw, gen, timings=True)
        torch.cuda.synchronize()
        if j >= 2:
            rows.append({"wall_ms": (time.perf_counter() - t0) * 1e3, "added": int(res["added"]), **res["timings_ms"]})
    return rows


if args.draws_only:
    # (a model's first keyframe: rend_alpha = None, every valid pixel a candidate — the largest k a keyframe can ask for)
    cam = frames[n_kf].camera
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    for i in range(args.draws_only):
        pixels, _ = fused_mapper._densify_draw_device(cam, None, 0.5, 0.15, 0, i)
        drawn, _ = fused_mapper._densify_draw_hip(cam, None, 0.5, 0.15, gen)
        drawn.reshape(-1).nonzero()
    torch.cuda.synchronize()
    print(f"{args.draws_only} draws of {int(pixels.numel())} pixels each way")
    sys.exit(0)

if args.ab:
    block("torch", 1); block("device", 1)              # the process's own first launches
    per = {"torch": [], "device": []}
    for b in range(args.blocks):
        for draw in (("torch", "device") if b % 2 == 0 else ("device", "torch")):
            per[draw].append(block(draw))
    stages = [s for s in per["torch"][0][0] if s != "added"]
    out = {"workload": f"{n0} surfels + 15 % of the candidates per keyframe, {H}x{W}, window of {n_kf}, num_iterations {iters}; "
                       f"{args.blocks} interleaved blocks per draw, 4 timed keyframes per block, each block on a fresh model",
           "ratio": "wall_ms / the `iterations` stage of the same update_model call"}
    for draw, blocks in per.items():
        med = {s: [float(np.median([r[s] for r in rows])) for rows in blocks] for s in stages}
        ratio = [float(np.median([r["wall_ms"] / r["iterations"] for r in rows])) for rows in blocks]
        out[draw] = {"median_ms": {s: round(float(np.median(x)), 4) for s, x in med.items()},
                     "block_medians_ms": {"densify_render_and_draw": [round(x, 4) for x in med["densify_render_and_draw"]],
                                          "wall_ms": [round(x, 3) for x in med["wall_ms"]]},
                     "wall_over_iterations": round(float(np.median(ratio)), 4),
                     "added": [int(r["added"]) for r in blocks[0]]}
    t, g = out["torch"]["median_ms"]["densify_render_and_draw"], out["device"]["median_ms"]["densify_render_and_draw"]
    out["densify_render_and_draw_ms"] = {"torch": t, "device": g, "saved": round(t - g, 4)}
    print(json.dumps(out, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    sys.exit(0)

model, kfs = fresh_model(), frames[:n_kf]
gen = torch.Generator(device=dev); gen.manual_seed(0)
for k in range(n_kf, n_kf + 2):
    kfs = kfs[1:] + [frames[k]]
    update(model, kfs, k, args.draw, gen)
torch.cuda.synchronize()
pr = cProfile.Profile()
pr.enable()
for k in range(n_kf + 2, n_kf + 6):
    kfs = kfs[1:] + [frames[k]]
    update(model, kfs, k, args.draw, gen)
torch.cuda.synchronize()
pr.disable()
st = pstats.Stats(pr)
st.sort_stats("cumulative").print_stats(45)
