#!/usr/bin/env python3
"""Times the ground segmentation (splat_loam_amd.evaluation.segment_ground -> sls_ground_segment) on the synthetic street scan
of tests/ground_ref.py, against the rule's two other statements, after checking that all three give the same bits:

    python tools/ground_bench.py [--reps 10] [--out profiles/r25a_ground.json] [--no-stages]

  scans        the street at 64 x 2048 returns (about 130 k points) and at 16 x 1024.
  native       the whole call: device tensor in, mask / bins / planes / info / status out, torch.cuda.synchronize inside the
               timed region.
  host_serial  include/sls_ground_math.h's serial whole-cloud routine (the 64 lanes emulated), compiled here with gcc -O2
               -ffp-contract=off into a shared object, on ONE host core, the copy of the scan down to the host and of the
               labels back up included.
  numpy        the restatement tests/ground_ref.py, the same copies included.
  stages       the native call's kernels by stage — keys (init + keys), sort (the 41-bit LSD sort's histogram, row scan and
               scatter launches), gather, fit — from `rocprofv3 --kernel-trace --stats` over a CHILD process of this tool
               that runs the call alone (a run of its own: tracing slows the host, so no end-to-end number comes from it).
  projector    DeviceProjector.scan_to_images at 64 x 2048 with and without ground=True, against each other.
Native, host_serial and numpy run in one process and alternate; 3 warm-ups, the median of --reps (>= 10).  The parent commit has
no such path and Patchwork itself is not installed, so there is no ratio to meet: the file says what was measured."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import ground_ref as ref
from outlier_bench import alternate
from splat_loam_amd import _abi, evaluation, projector

SCANS = ((64, 2048), (16, 1024))
WRAPPER = r'''
#include "sls_ground_math.h"
int ground_host(int M, const float *xyz, const SlsGroundParams *p, uint8_t *label, int32_t *bin, double *planes, int32_t *info,
                uint32_t *status) { return sls_ground_segment_host(M, xyz, p, label, bin, planes, info, status); }
'''
STAGES = (("keys", ("ground_init_kernel", "ground_keys_kernel")), ("sort", ("sort_hist_kernel", "sort_rowscan_kernel", "sort_scatter_kernel")),
          ("gather", ("ground_gather_kernel",)), ("fit", ("ground_fit_kernel",)))


def host_library(tmp):
    src = os.path.join(tmp, "ground_host.c")
    with open(src, "w") as f:
        f.write(WRAPPER)
    so = os.path.join(tmp, "ground_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.ground_host.restype = C.c_int
    lib.ground_host.argtypes = [C.c_int, C.c_void_p, C.POINTER(_abi.SlsGroundParams)] + [C.c_void_p] * 5
    return lib


def host_serial(lib, prm, cloud_dev):
    pts = cloud_dev.cpu().numpy()                                       # the copy down
    M = len(pts)
    label, bins = np.empty(M, np.uint8), np.empty(M, np.int32)
    planes, info, status = np.empty((ref.BINS, 8)), np.empty((ref.BINS, 4), np.int32), np.empty(8, np.uint32)
    rc = lib.ground_host(M, pts.ctypes.data, C.byref(prm), label.ctypes.data, bins.ctypes.data, planes.ctypes.data, info.ctypes.data,
                         status.ctypes.data)
    assert rc == 0
    return torch.from_numpy(label).to(cloud_dev.device), bins, planes, info, status    # the copy up


def numpy_side(cloud_dev):
    res = ref.segment(cloud_dev.cpu().numpy())
    return torch.from_numpy(res["label"]).to(cloud_dev.device), res["bin"], res["planes"], res["info"], res["status"]


def kernel_stages(H, W, calls, tmp):
    """{stage: us per call} from rocprofv3's kernel statistics of a child process that runs the call alone"""
    if shutil.which("rocprofv3") is None:
        return {"not_measured": "rocprofv3 is not installed"}
    out = os.path.join(tmp, f"trace_{H}x{W}")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "g", "--", sys.executable,
           os.path.abspath(__file__), "--trace-child", str(H), str(W), str(calls)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if done.returncode != 0 or not files:
        return {"not_measured": f"rocprofv3 ended with {done.returncode}: {done.stderr[-300:]}"}
    total = {name: 0.0 for name, _ in STAGES}
    for row in csv.DictReader(open(files[0])):
        for name, kernels in STAGES:
            if any(k in row["Name"] for k in kernels):
                total[name] += float(row["AverageNs"]) * float(row["Calls"])
    # (the child's warm-up calls are traced too: every call is the same work)
    return {name: round(ns / 1e3 / (calls + 3), 2) for name, ns in total.items()}


def trace_child(H, W, calls):
    dev = torch.device("cuda:0")
    cloud = torch.from_numpy(ref.street(H, W, seed=1)[0]).to(dev)
    for _ in range(calls + 3):
        evaluation.segment_ground(cloud, return_details=True)
    torch.cuda.synchronize(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25a_ground.json"))
    ap.add_argument("--no-stages", action="store_true", help="skip the rocprofv3 child runs")
    ap.add_argument("--trace-child", nargs=3, type=int, metavar=("H", "W", "CALLS"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ground_bench needs a GPU: a time taken elsewhere says nothing")
    if a.trace_child:
        return trace_child(*a.trace_child)
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    dev = torch.device("cuda:0")
    prm = evaluation._check_ground_args(1.723, {})
    res = {"what": "evaluation.segment_ground (sls_ground_segment) against the header's serial routine on one host core and the "
                   "NumPy restatement, equal outputs asserted first; DeviceProjector.scan_to_images with and without ground=True",
           "data": "synthetic street (tests/ground_ref.py: street, seed 1), defaults",
           "protocol": f"one process, the sides alternating, 3 warm-ups, median of {a.reps}, torch.cuda.synchronize inside the timed "
                       "region; host sides include the copy of the scan down and of the labels up; stages from rocprofv3 "
                       "--kernel-trace --stats over a child process that runs the native call alone",
           "device": torch.cuda.get_device_name(0), "scans": []}
    with tempfile.TemporaryDirectory() as tmp:
        lib = host_library(tmp)
        for H, W in SCANS:
            pts, truth = ref.street(H, W, seed=1)
            cloud = torch.from_numpy(pts).to(dev)
            native = lambda: evaluation.segment_ground(cloud, return_details=True)      # noqa: E731
            got = [t.cpu().numpy() for t in native()]
            for name, other in (("host_serial", host_serial(lib, prm, cloud)), ("numpy", numpy_side(cloud))):
                assert np.array_equal(got[0], other[0].cpu().numpy() != 0), f"{name}: labels differ"
                assert np.array_equal(got[1], other[1]) and np.array_equal(got[3], other[3]), f"{name}: bins or info differ"
                assert np.array_equal(got[2].view(np.uint64), other[2].view(np.uint64)), f"{name}: planes differ"
                assert np.array_equal(got[4].view(np.uint32), other[4]), f"{name}: status differ"
            use = got[1] >= 0
            tp = int((got[0] & truth)[use].sum())
            run = {"H": H, "W": W, "points": len(pts), "with_bin": int(use.sum()), "ground_found": int(got[0].sum()),
                   "precision": round(tp / max(int(got[0][use].sum()), 1), 4), "recall": round(tp / max(int(truth[use].sum()), 1), 4),
                   "bin_states": dict(zip(evaluation.GROUND_STATES, np.bincount(got[3][:, 3], minlength=6).tolist())),
                   "outputs_equal": True}
            run["native_ms"], run["host_serial_ms"], run["numpy_ms"] = alternate(
                [native, lambda: host_serial(lib, prm, cloud), lambda: numpy_side(cloud)], a.reps, dev)
            run["stage_us"] = {"not_measured": "--no-stages"} if a.no_stages else kernel_stages(H, W, a.reps, tmp)
            res["scans"].append(run)
        H, W = SCANS[0]
        cloud = torch.from_numpy(ref.street(H, W, seed=1)[0]).to(dev)
        plain, ground = (projector.DeviceProjector(H, W, 0.5, 100.0, device=dev, ground=g) for g in (False, True))
        a_img, b_img = plain.scan_to_images(cloud), ground.scan_to_images(cloud)
        assert all(torch.equal(a_img[k], b_img[k]) for k in ("lut", "range_image", "valid"))
        t_plain, t_ground = alternate([lambda: plain.scan_to_images(cloud), lambda: ground.scan_to_images(cloud)], a.reps, dev)
        res["projector"] = {"H": H, "W": W, "points": int(cloud.shape[0]), "ground_pixels": int(b_img["ground"].sum()),
                            "scan_to_images_ms": t_plain, "scan_to_images_ground_ms": t_ground,
                            "ground_costs_ms": round(t_ground["median"] - t_plain["median"], 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
