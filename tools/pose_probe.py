#!/usr/bin/env python
"""What the pose gradient costs, and the model-frozen refinement at full size.

    python tools/pose_probe.py [--out FILE.json] [--steps 40] [--no-refine]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pose_probe.py --trace-only     # preprocess_bwd alone

Times MappingEngine.step with and without pose_grad=True (status read every iteration in both: the flag needs it), and
pose_step, at BASELINE config 3 (500 000 surfels, 64 x 2048) and at 50 000 / 64 x 1024, interleaved in blocks so that
clock drift hits both alike; then runs pose.refine_pose on the box room of tests/pose_ref.py at 64 x 1024 with a 0.065 m
grid (about 50 000 surfels).  No bars: the figures go to profiles/.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch


def engine_for(N, H, W, seed=0):
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    sc = synth.make_scene(N, H, W, seed=seed)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, synth.keyframe_poses(2)[1], data_device="cuda:0")
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
    return MappingEngine(model, MappingConfig()), cam


def time_steps(N, H, W, steps, blocks=4):
    eng, cam = engine_for(N, H, W)
    for _ in range(5):
        eng.step(cam)
        eng.step(cam, pose_grad=True)
        eng.pose_step(cam)
    kinds = {"step": lambda: eng.step(cam), "step_pose_grad": lambda: eng.step(cam, pose_grad=True),
             "pose_step": lambda: eng.pose_step(cam)}
    ms = {k: [] for k in kinds}
    for _ in range(blocks):
        for k, fn in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    out = {k: {"ms_per_iteration_blocks": v, "median_ms": float(np.median(v))} for k, v in ms.items()}
    out["pose_grad_extra_us"] = 1e3 * (out["step_pose_grad"]["median_ms"] - out["step"]["median_ms"])
    out["repeated"] = dict(eng.stats)
    return out


def trace_only(steps):
    """A short run for a kernel trace: the same number of iterations with and without the reduction"""
    for N, H, W in ((500000, 64, 2048), (50000, 64, 1024)):
        eng, cam = engine_for(N, H, W)
        for _ in range(steps):
            eng.step(cam)
        for _ in range(steps):
            eng.step(cam, pose_grad=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--no-refine", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    if args.trace_only:
        trace_only(args.steps)
        return
    res = {"device": torch.cuda.get_device_name(0), "timing": {}}
    for N, H, W in ((500000, 64, 2048), (50000, 64, 1024)):
        res["timing"][f"{N}@{H}x{W}"] = time_steps(N, H, W, args.steps)
        print(json.dumps({f"{N}@{H}x{W}": res["timing"][f"{N}@{H}x{W}"]}), flush=True)
    if not args.no_refine:
        import pose_ref
        r = pose_ref.run_refinement(torch.device("cuda:0"), H=64, W=1024, step=0.065)
        res["refinement_64x1024"] = r
        print(json.dumps({"refinement_64x1024": {k: v for k, v in r.items() if k not in ("refined", "negated")},
                          "refined": {k: v for k, v in r["refined"].items() if k != "loss"},
                          "negated": {k: v for k, v in r["negated"].items() if k != "loss"}}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
