"""The surface sampler without a GPU ("Surface samples"): the header's sls_sample_word /
sls_sample_index compiled for the host against the NumPy restatement (tests/surface_ref.py) bit for bit, the ranks'
range and distribution, the keyframe interval rule against a transcription of the reference's loop, the point-cloud
writer, and the new C-ABI entry points' host-side behaviour."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import surface_ref as ref
from splat_loam_amd import _abi, meshing, ply_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "sls_draw_math.h"
/* OUT SEED FRAME N_SAMPLES N_VALID : per sample (random word, rank) */
int main(int argc, char **argv)
{
    if (argc < 6) return 2;
    FILE *out = fopen(argv[1], "wb");
    if (!out) return 3;
    const uint64_t seed = strtoull(argv[2], 0, 10);
    const uint32_t frame = (uint32_t)strtoul(argv[3], 0, 10), n = (uint32_t)strtoul(argv[4], 0, 10);
    const uint32_t n_valid = (uint32_t)strtoul(argv[5], 0, 10);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t r = sls_sample_word(j, seed, frame);
        uint32_t o[2] = { r, sls_sample_index(r, n_valid) };
        fwrite(o, 4, 2, out);
    }
    fclose(out);
    return 0;
}
"""

SEED = 0x9E3779B97F4A7C15          # a 64-bit seed: both key words are in use
FRAME = 4242


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """include/sls_draw_math.h compiled with the host compiler under the header's own rule (-ffp-contract=off)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("surface_math")
    src = d / "driver.c"
    src.write_text(_DRIVER)
    exe = d / "driver"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return str(exe), d


def _header(driver, n_samples, n_valid, seed=SEED, frame=FRAME):
    exe, d = driver
    out = d / f"s_{n_samples}_{n_valid}.bin"
    subprocess.check_call([exe, str(out), str(seed), str(frame), str(n_samples), str(n_valid)])
    got = np.fromfile(out, dtype=np.uint32).reshape(-1, 2)
    return got[:, 0], got[:, 1]


@pytest.mark.parametrize("n_valid", [1, 2, 63, 64, 65, 16650, 262144])
def test_header_equals_numpy_bit_for_bit(driver, n_valid):
    """10^4 samples: the random words and the ranks of the header equal the restatement's; every rank is < n_valid."""
    words, idx = _header(driver, 10000, n_valid)
    want_words = ref.sample_words(10000, SEED, FRAME)
    assert np.array_equal(words, want_words)
    want_idx = ref.sample_indices(want_words, n_valid)
    assert np.array_equal(idx, want_idx)
    assert int(idx.max()) < n_valid and int(want_idx.max()) < n_valid
    if n_valid == 1:
        assert not idx.any()


def test_stream_is_disjoint_from_the_densify_draw():
    """Counter word 1 is 1 here and 0 in the densify draw: the same (index, seed, third word) give other words."""
    import densify_draw_ref
    assert not np.array_equal(ref.sample_words(64, SEED, 7), densify_draw_ref.draw_words(64, SEED, 7))
    assert not np.array_equal(ref.sample_words(64, SEED, 7), ref.sample_words(64, SEED, 8))
    assert not np.array_equal(ref.sample_words(64, SEED, 7), ref.sample_words(64, SEED + 1, 7))


def test_ranks_are_uniform(driver):
    """2 10^5 samples at n_valid = 1000: Pearson's chi-square of the bin counts (999 degrees of freedom) is within its
    99.9 % quantile, 1142.85 — computed here by Wilson-Hilferty, 999 (1 - 2/(9 999) + 3.0902 sqrt(2/(9 999)))^3 = 1142.9
    (the approximation is good to 0.1 at this many degrees of freedom).  The seed is fixed, so is the outcome: 1016.5."""
    n, bins = 200000, 1000
    _, idx = _header(driver, n, bins)
    counts = np.bincount(idx, minlength=bins)
    assert counts.size == bins
    chi2 = float(((counts - n / bins) ** 2 / (n / bins)).sum())
    df = bins - 1
    q999 = df * (1.0 - 2.0 / (9.0 * df) + 3.0902 * np.sqrt(2.0 / (9.0 * df))) ** 3
    print(f"chi2 = {chi2:.1f}, 99.9 % quantile = {q999:.1f}")
    assert chi2 <= q999


def _reference_loop(models, kf_interval):
    """scene/postprocessing.py:123-140, transcribed: the frames that are NOT skipped."""
    used = []
    processed_frames = 0
    for rmodel in models:
        for rfid in rmodel["frame_ids"]:
            processed_frames += 1
            if kf_interval is not None and kf_interval > 0 and \
                    (processed_frames % kf_interval):
                continue
            used.append(rfid)
    return used


@pytest.mark.parametrize("kf_interval", [-1, 0, 1, 2, 3])
def test_interval_rule_is_the_references(kf_interval):
    graph = {"models": [{"id": 0, "frame_ids": [0, 1, 2]}, {"id": 1, "frame_ids": [3, 4, 5]}]}
    got = meshing.frames_to_sample(graph, kf_interval)
    assert [fid for _, fid in got] == _reference_loop(graph["models"], kf_interval)
    assert [mi for mi, _ in got] == [0 if fid < 3 else 1 for _, fid in got]
    want = {-1: [0, 1, 2, 3, 4, 5], 0: [0, 1, 2, 3, 4, 5], 1: [0, 1, 2, 3, 4, 5], 2: [1, 3, 5], 3: [2, 5]}[kf_interval]
    assert [fid for _, fid in got] == want           # (the counter runs across the models and starts at 1)


def _read_cloud(path):
    """A ten-line PLY reader: header names in order, then the float32 rows."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = [ln.split() for ln in lines if ln.startswith("element")]
    props = [ln.split() for ln in lines if ln.startswith("property")]
    n = int(elements[0][2])
    rows = np.frombuffer(blob, dtype="<f4", count=n * len(props), offset=end).reshape(n, len(props))
    assert end + rows.nbytes == len(blob)
    return elements, props, rows


def test_save_point_cloud_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(37, 3)).astype(np.float32) * 50
    nrm = rng.normal(size=(37, 3)).astype(np.float32)
    path = tmp_path / "sub" / "cloud.ply"
    ply_io.save_point_cloud(path, pts, nrm)
    elements, props, rows = _read_cloud(path)
    assert elements == [["element", "vertex", "37"]]
    assert [p[2] for p in props] == ["x", "y", "z", "nx", "ny", "nz"] and all(p[1] == "float" for p in props)
    assert np.array_equal(rows[:, :3], pts) and np.array_equal(rows[:, 3:], nrm)
    import torch
    ply_io.save_point_cloud(path, torch.from_numpy(pts), torch.from_numpy(nrm))          # tensors too
    assert np.array_equal(_read_cloud(path)[2], np.concatenate([pts, nrm], 1))
    ply_io.save_point_cloud(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert _read_cloud(path)[2].shape == (0, 6)
    with pytest.raises(ValueError):
        ply_io.save_point_cloud(path, pts, nrm[:5])


def test_surface_samples_abi_errors_host_side():
    """SLS_E_ARG / SLS_E_UNSUPPORTED before anything is enqueued, without a GPU."""
    lib = _abi.lib()
    H, W = 50, 333
    need = lib.sls_surface_scratch_bytes(H, W)
    assert need >= (H * W + 7) // 8
    assert lib.sls_surface_scratch_bytes(256, 1024) >= (1 << 18) // 8 > need           # the cap itself is served
    assert lib.sls_surface_scratch_bytes(0, W) == 0 and lib.sls_surface_scratch_bytes(H, -1) == 0
    fake = (C.c_uint8 * 64)()                     # a non-null, aligned address: no call below gets as far as using it
    p = (C.addressof(fake) + 15) & ~15
    nan = float("nan")

    def call(H=H, W=W, allmap=p, col=p, row=p, M=p, min_op=0.5, max_dd=0.1, ratio=0.0, n=100, pts=p, nrm=p, pix=None, status=p,
             scratch=p, nbytes=need):
        return lib.sls_surface_samples(H, W, allmap, col, row, M, min_op, max_dd, ratio, n, 1, 0, pts, nrm, pix, status, scratch,
                                       nbytes, None)

    for kw, word in (({"allmap": None}, b"null pointer"), ({"col": None}, b"null pointer"), ({"row": None}, b"null pointer"),
                     ({"M": None}, b"null pointer"), ({"pts": None}, b"null pointer"), ({"nrm": None}, b"null pointer"),
                     ({"status": None}, b"null pointer"), ({"scratch": None}, b"null pointer"),
                     ({"H": 0}, b"size"), ({"W": -3}, b"size"), ({"n": 0}, b"n_samples"), ({"n": -5}, b"n_samples"),
                     ({"min_op": nan}, b"NaN"), ({"max_dd": nan}, b"NaN"), ({"ratio": nan}, b"NaN"),
                     ({"nbytes": need - 1}, b"scratch"), ({"nbytes": 0}, b"scratch"), ({"scratch": p + 4}, b"aligned")):
        assert call(**kw) == -1, kw                                            # SLS_E_ARG
        assert word in lib.sls_last_error(), (kw, lib.sls_last_error())
        with pytest.raises(RuntimeError, match="sls_surface_samples"):
            _abi.check(-1, "sls_surface_samples")
    assert call(H=512, W=1024, nbytes=lib.sls_surface_scratch_bytes(512, 1024)) == -4      # SLS_E_UNSUPPORTED: 2^19 pixels
    assert b"262144" in lib.sls_last_error()


def test_python_side_refuses_what_it_does_not_serve(tmp_path):
    import torch
    with pytest.raises(RuntimeError, match="ROCm device"):
        meshing.sample_keyframe(torch.zeros((7, 8, 64)), None, np.eye(4))
    from splat_loam_amd import traj_io
    traj_io.write_graph(tmp_path / "graph.yaml", [], [])
    with pytest.raises(ValueError, match="image size"):
        meshing.sample_surface(tmp_path)
    with pytest.raises(RuntimeError, match="ROCm device"):
        meshing.sample_surface(tmp_path, device="cpu", image_height=8, image_width=64)
