#!/usr/bin/env python3
"""Stress of the depth-order repair at awkward sizes: for several surfel counts (below one window, window edges, odd)
and one to four repair rounds the repaired order must equal the from-scratch order bit for bit, with the loss stage
inside the tile backward and without (deterministic accumulation, so that every configuration walks the same
trajectory).  python tools/repair_fuzz.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from splat_loam_amd import synth
from splat_loam_amd.engine import MappingEngine
from splat_loam_amd.mapping import MappingConfig
from splat_loam_amd.scene import Camera, SurfelModel


def run(dev="cuda:0", verbose=True):
    bad = 0
    for N, H, W in ((700, 32, 256), (1024, 32, 256), (1025, 32, 256), (1536, 16, 128), (2049, 40, 200), (30001, 64, 512), (65536, 64, 1024)):
        sc = synth.make_scene(N, H, W, seed=N, range_lo=2.0, range_hi=25.0)
        depth, valid = synth.make_targets(H, W, sc)
        cam = Camera(sc["K"], depth, None, valid, None, data_device=dev)
        ref = None
        for rounds in (0, 1, 2, 3, 4):
            for inline in (True, False):
                m = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=dev)
                e = MappingEngine(m, MappingConfig())
                e.reuse_depth_order = rounds > 0
                e.deterministic = True            # (bit-identical trajectories: the orders can be compared at all)
                e.inline_loss_stage = inline
                e._repair_rounds, e._repair_until = max(rounds, 1), 10 ** 9
                losses = [e.step(cam)["loss"] for _ in range(4)]
                order = e._orders[id(cam)].order.cpu().numpy()
                params = [p.detach().cpu().numpy() for p in (m._xyz, m._scaling, m._rotation, m._opacity)]
                if ref is None:
                    ref = (order, losses, params)
                else:
                    ok = np.array_equal(order, ref[0]) and np.allclose(losses, ref[1], rtol=1e-5) and e.stats["repeated_resort"] == 0
                    drift = max(float(np.abs(a - b).max()) for a, b in zip(params, ref[2]))
                    if not ok or drift != 0.0:
                        bad += 1
                        print("MISMATCH", N, H, W, rounds, inline, e.stats, drift, losses, ref[1])
        if verbose:
            print(f"{N} surfels {H}x{W}: ok" if bad == 0 else f"{N}: {bad} mismatches so far")
    if verbose:
        print("repair fuzz:", "all orders identical" if bad == 0 else f"{bad} mismatches")
    return bad


if __name__ == "__main__":
    sys.exit(1 if run() else 0)
