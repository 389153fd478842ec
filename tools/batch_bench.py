"""Keyframe-batched mapping step (MappingEngine.step_batch): ms per step and per keyframe for G in {1, 2, 4, 8} at
C3 (500 k surfels, 64x2048) and at 170 k / 64x1024, on the same keyframe poses (synth.keyframe_poses(8)); and, for
comparison, step() over the same eight keyframes in turn (status read every iteration / lagged).
Prints one JSON line.

    python tools/batch_bench.py [--steps 30] [--warmup 5] [--sizes c3,170k] [--gs 1,2,4,8]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"c3": (500000, 64, 2048), "170k": (170000, 64, 1024)}


def run(N, H, W, gs, steps, warmup, modes=("batch", "sync", "lagged")):
    import torch
    from splat_loam_amd import synth
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import Camera, SurfelModel
    sc = synth.make_scene(N, H, W, seed=0, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    poses = synth.keyframe_poses(8)
    cams = [Camera(sc["K"], depth, None, valid, poses[k], data_device="cuda:0") for k in range(8)]
    out = {}
    for G in (gs if "batch" in modes else ()):
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
        eng = MappingEngine(model, MappingConfig())
        batch = cams[:G]
        for _ in range(warmup):           # (capacity and the keyframes' orders settle; every status read)
            eng.step_batch(batch)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        void = 0
        for _ in range(steps):
            void += bool(eng.step_batch(batch)["overflow"])      # (never: a void batch is repeated inside)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / steps
        out[f"G{G}"] = {"ms_per_step": round(ms, 4), "ms_per_keyframe": round(ms / G, 4), "repeats": dict(eng.stats),
                        "void": void}
        del eng, model
        torch.cuda.empty_cache()
    # what a caller has without the batch: step() over the same keyframes in turn, one update per keyframe — with a
    # status read per iteration (as the batch above) and lagged (the engine's fastest single-keyframe mode)
    G = max(gs)
    for mode in [m for m in ("sync", "lagged") if m in modes]:
        model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
        eng = MappingEngine(model, MappingConfig())
        sync = True if mode == "sync" else "lagged"
        for i in range(warmup * G):
            eng.step(cams[i % G], sync=sync)
        eng.flush()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for i in range(steps * G):
            eng.step(cams[i % G], sync=sync)
        eng.flush()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / (steps * G)
        out[f"step_{mode}_over_{G}"] = {"ms_per_keyframe": round(ms, 4), "repeats": dict(eng.stats)}
        del eng, model
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="c3,170k")
    ap.add_argument("--gs", default="1,2,4,8")
    ap.add_argument("--modes", default="batch,sync,lagged", help="batch: step_batch per G; sync / lagged: step() over max(G) keyframes")
    a = ap.parse_args()
    gs = [int(g) for g in a.gs.split(",")]
    res = {"metric": "keyframe-batched mapping step", "unit": "ms", "steps": a.steps, "warmup": a.warmup,
           "sync": "every step reads its status (sync=True: the keyframes' depth orders are repaired)", "sizes": {}}
    for name in a.sizes.split(","):
        N, H, W = SIZES[name]
        res["sizes"][name] = {"N": N, "H": H, "W": W, **run(N, H, W, gs, a.steps, a.warmup, a.modes.split(","))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
