"""The seeded densify draw without a GPU ("The densify draw"): Philox4x32-10's known answers, the
header include/sls_draw_math.h compiled for the host against the NumPy restatement (tests/densify_draw_ref.py) bit for
bit, the accuracy of its -ln(u) over every possible u, the draw's distribution against torch.multinomial, and the new
C-ABI entry points' host-side behaviour."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import densify_draw_ref as ref
from splat_loam_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "sls_draw_math.h"
/* words  IN OUT          : uint32 words -> per word (bits of u, bits of E)
 * all    OUT             : E(u) for the 2^23 values of u, in order of r >> 9
 * keys   IN OUT SEED IDX : float32 weights -> per pixel (random word, bits of the key)
 * philox c0 c1 c2 c3 k0 k1 (hex) : the four output words */
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "philox")) {
        uint32_t c[4];
        for (int i = 0; i < 4; ++i) c[i] = (uint32_t)strtoul(argv[2 + i], 0, 16);
        sls_philox4x32_10(c, (uint32_t)strtoul(argv[6], 0, 16), (uint32_t)strtoul(argv[7], 0, 16));
        printf("%08x %08x %08x %08x\n", c[0], c[1], c[2], c[3]);
        return 0;
    }
    if (!strcmp(argv[1], "all")) {
        FILE *out = fopen(argv[2], "wb");
        if (!out) return 3;
        for (uint32_t i = 0; i < (1u << 23); ++i) {
            const float E = sls_draw_neg_log(sls_draw_uniform(i << 9));
            fwrite(&E, 4, 1, out);
        }
        fclose(out);
        return 0;
    }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    if (!strcmp(argv[1], "words")) {
        uint32_t r;
        while (fread(&r, 4, 1, in) == 1) {
            const float u = sls_draw_uniform(r);
            uint32_t o[2] = { sls_draw_float_bits(u), sls_draw_float_bits(sls_draw_neg_log(u)) };
            fwrite(o, 4, 2, out);
        }
    } else {
        const uint64_t seed = strtoull(argv[4], 0, 10);
        const uint32_t idx = (uint32_t)strtoul(argv[5], 0, 10);
        float w;
        for (uint32_t p = 0; fread(&w, 4, 1, in) == 1; ++p) {
            const uint32_t r = sls_draw_word(p, seed, idx);
            uint32_t o[2] = { r, sls_draw_float_bits(sls_draw_key(w, r)) };
            fwrite(o, 4, 2, out);
        }
    }
    fclose(in); fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """include/sls_draw_math.h compiled with the host compiler under the header's own rule (-ffp-contract=off)."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("draw_math")
    src = d / "driver.c"
    src.write_text(_DRIVER)
    exe = d / "driver"
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return str(exe), d


KNOWN = (
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


def test_philox_known_answers(driver):
    """The Random123 known-answer vectors of Philox4x32-10, from the NumPy restatement and from the header."""
    exe, _ = driver
    for ctr, key, want in KNOWN:
        got = " ".join(f"{int(x[0]):08x}" for x in ref.philox4x32_10(ctr, key))
        assert got == want
        out = subprocess.check_output([exe, "philox"] + [f"{v:x}" for v in ctr + key], text=True).strip()
        assert out == want


def test_header_equals_numpy_bit_for_bit(driver):
    """u and E over 2^20 random words and the edge words; the pixels' random words and race keys for a weight vector with
    zeros, the 1e-30 floor, tiny and large weights, under a 64-bit seed and a draw index."""
    exe, d = driver
    rng = np.random.default_rng(11)
    words = np.concatenate([np.array([0, 0x1FF, 0x200, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000, 0xB504F200, 0xB504F400], np.uint32),
                            rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)])
    words.tofile(d / "words.bin")
    subprocess.check_call([exe, "words", str(d / "words.bin"), str(d / "words.out")])
    got = np.fromfile(d / "words.out", dtype=np.uint32).reshape(-1, 2)
    u = ref.uniform(words)
    assert np.array_equal(got[:, 0], u.view(np.uint32))
    assert np.array_equal(got[:, 1], ref.neg_log(u).view(np.uint32))
    assert float(u.min()) == 2.0 ** -24 and float(u.max()) == 1.0 - 2.0 ** -24          # never 0 or 1

    n = 1 << 16
    w = np.exp(rng.normal(size=n) * 4.0).astype(np.float32)
    w[rng.random(n) < 0.2] = 0.0
    w[rng.random(n) < 0.1] = np.float32(1.0e-30)
    w[:4] = np.array([0.0, 1.0e-30, 1.0e-12, 3.0e4], np.float32)
    w.tofile(d / "w.bin")
    seed, idx = 0xFEDCBA9876543210, 0x89ABCDEF
    subprocess.check_call([exe, "keys", str(d / "w.bin"), str(d / "keys.out"), str(seed), str(idx)])
    got = np.fromfile(d / "keys.out", dtype=np.uint32).reshape(-1, 2)
    assert np.array_equal(got[:, 0], ref.draw_words(n, seed, idx))
    keys = ref.keys(w, seed, idx)
    assert np.array_equal(got[:, 1], keys.view(np.uint32))
    assert bool(np.isinf(keys[w == 0]).all()) and bool(np.isfinite(keys[w > 0]).all())
    # a zero-gradient candidate's key lies above every positive-weight candidate's (E >= 2^-24, w = 1e-30 against E <= 17, w)
    floor = w == np.float32(1.0e-30)
    assert float(keys[floor].min()) > float(keys[(w > 0) & ~floor].max())


def test_neg_log_accuracy_over_every_u(driver):
    """E = -ln(u) against float64 over all 2^23 values of u: relative error <= 1e-6, E > 0 everywhere — from the compiled
    header; the NumPy restatement gives the same bits."""
    exe, d = driver
    subprocess.check_call([exe, "all", str(d / "all.out")])
    E = np.fromfile(d / "all.out", dtype=np.float32)
    assert E.size == 1 << 23
    u = ref.uniform(np.arange(1 << 23, dtype=np.uint32) << np.uint32(9))
    assert np.array_equal(E.view(np.uint32), ref.neg_log(u).view(np.uint32))
    want = -np.log(u.astype(np.float64))
    rel = np.abs(E.astype(np.float64) - want) / want
    print(f"\n[draw math] -ln(u): largest relative error {rel.max():.3e} at u = {float(u[rel.argmax()])!r}; smallest E {E.min():.3e}")
    assert bool((E > 0).all())
    assert float(rel.max()) <= 1e-6


def test_draw_has_multinomials_distribution():
    """The reference draw over 12 weights (a 0 and a 1e-30 among them), k = 4, 40 000 seeds, against 40 000 draws of
    torch.multinomial (CPU, seeded): every pixel's inclusion frequency agrees within 4 sigma of the difference of two
    such frequencies at p = 0.5 (sigma = sqrt(2 * 0.25 / 40000) = 0.00354: bound 0.0141); the zero weight is never drawn."""
    w = np.array([0.5, 1.0, 2.0, 0.0, 1.0e-30, 3.0, 0.25, 1.5, 0.75, 4.0, 0.1, 1.0], np.float32)
    n, k, draws = w.size, 4, 40_000
    seeds = np.arange(draws, dtype=np.uint64) + np.uint64(1000)
    pix = np.arange(n, dtype=np.uint64)[None, :]
    zero = np.zeros_like(pix)
    words = ref.philox4x32_10((pix, zero, zero + np.uint64(7), zero), (seeds[:, None] & np.uint64(0xFFFFFFFF), seeds[:, None] >> np.uint64(32)))[0]
    E = ref.neg_log(ref.uniform(words.reshape(-1))).reshape(draws, n)
    keys = np.full((draws, n), np.inf, np.float32)
    keys[:, w > 0] = E[:, w > 0] / w[None, w > 0]
    composite = (keys.view(np.uint32).astype(np.uint64) << np.uint64(32)) | pix
    chosen = np.argsort(composite, axis=1, kind="stable")[:, :k]
    # (one row through the module's own entry point: the vectorised form above is the same draw)
    assert np.array_equal(np.sort(chosen[5]), ref.select(ref.keys(w, int(seeds[5]), 7), k))
    f_ref = np.bincount(chosen.reshape(-1), minlength=n) / draws
    gen = torch.Generator().manual_seed(1234)
    got = torch.multinomial(torch.tensor(w)[None, :].expand(draws, n).contiguous(), k, replacement=False, generator=gen).numpy()
    f_torch = np.bincount(got.reshape(-1), minlength=n) / draws
    diff = np.abs(f_ref - f_torch)
    print(f"\n[draw distribution] inclusion frequencies, race vs torch.multinomial: largest difference {diff.max():.4f} "
          f"(bound 0.0141); race {np.round(f_ref, 4).tolist()}")
    assert f_ref[3] == 0.0 and f_torch[3] == 0.0
    assert float(diff.max()) <= 0.0141
    assert abs(f_ref.sum() - k) < 1e-9


def test_new_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "sls_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sls_[a-z0-9_]+)\s*\(", src))
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ("sls_densify_draw", "sls_densify_draw_scratch_bytes"):
        assert name in declared, f"{name} not declared in sls_abi.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _abi.EXPORTS, f"{name} has no ctypes prototype"
    assert int(re.search(r"#define SLS_DENSIFY_DRAW_MAX_PIXELS (\d+)", src).group(1)) == 1 << 18


def test_argument_errors_never_touch_the_device():
    """Every argument error returns SLS_E_ARG with a message before anything is enqueued (this process has no GPU), an
    image beyond 2^18 pixels SLS_E_UNSUPPORTED; the scratch size grows with H * W."""
    lib = _abi.lib()
    H, W = 64, 1024
    need = lib.sls_densify_draw_scratch_bytes(H, W)
    assert need >= H * W * 4
    assert lib.sls_densify_draw_scratch_bytes(128, 1024) > need > lib.sls_densify_draw_scratch_bytes(50, 333) >= 50 * 333 * 4
    assert lib.sls_densify_draw_scratch_bytes(0, W) == 0 and lib.sls_densify_draw_scratch_bytes(H, -1) == 0
    fake = (C.c_uint8 * 64)()                     # a non-null, 16-byte aligned address: no call below gets as far as using it
    p = (C.addressof(fake) + 15) & ~15

    def call(H=H, W=W, depth=p, valid=p, alpha=None, pct=0.15, w=p, pix=p, stats=p, mirror=None, scratch=p, nbytes=need):
        return lib.sls_densify_draw(H, W, depth, valid, alpha, 0.5, pct, 1, 0, w, pix, stats, mirror, scratch, nbytes, None)

    for kw, word in (({"depth": None}, b"null pointer"), ({"valid": None}, b"null pointer"), ({"w": None}, b"null pointer"),
                     ({"pix": None}, b"null pointer"), ({"stats": None}, b"null pointer"), ({"scratch": None}, b"null pointer"),
                     ({"H": 0}, b"size"), ({"W": -3}, b"size"),
                     ({"pct": -0.01}, b"percentage"), ({"pct": 1.01}, b"percentage"), ({"pct": float("nan")}, b"percentage"),
                     ({"nbytes": need - 1}, b"scratch"), ({"nbytes": 0}, b"scratch"), ({"scratch": p + 4}, b"aligned")):
        assert call(**kw) == -1, kw                                            # SLS_E_ARG
        assert word in lib.sls_last_error(), (kw, lib.sls_last_error())
        with pytest.raises(RuntimeError, match="sls_densify_draw"):
            _abi.check(-1, "sls_densify_draw")
    assert call(H=512, W=1024, nbytes=lib.sls_densify_draw_scratch_bytes(512, 1024)) == -4      # SLS_E_UNSUPPORTED: 2^19 pixels
    assert b"262144" in lib.sls_last_error()
    assert lib.sls_densify_draw_scratch_bytes(256, 1024) >= (1 << 18) * 4                       # the cap itself is served


def test_update_model_device_draw_refuses_what_it_does_not_serve():
    """draw="device" on CPU tensors raises before anything runs (there is no fall-back to torch's draw), and so do a
    generator or a mask passed along with it and an unknown draw; SLS_DEVICE_DRAW=1 leaves CPU tensors on today's path."""
    from types import SimpleNamespace
    from splat_loam_amd import fused_mapper, synth
    from splat_loam_amd.scene import Camera
    H, W = 8, 16
    cam = Camera(synth.spherical_K(H, W), np.full((1, H, W), 5.0, np.float32), None, np.ones((1, H, W), np.uint8), np.eye(4),
                 data_device="cpu")
    frame = SimpleNamespace(camera=cam, model_T_frame=torch.eye(4))
    mapping = SimpleNamespace(num_iterations=1, densify_threshold_egeom=-1.0, densify_threshold_opacity=0.5, densify_percentage=0.15,
                              prob_view_last_keyframe=0.4, pruning_min_opacity=0.0, pruning_min_size=0.0)
    cfg = SimpleNamespace(mapping=mapping, opt=SimpleNamespace(depth_ratio=0.0))
    with pytest.raises(RuntimeError, match="ROCm device"):
        fused_mapper.update_model(None, [frame], frame, cfg, draw="device")
    with pytest.raises(ValueError, match="generator"):
        fused_mapper.update_model(None, [frame], frame, cfg, draw="device", generator=torch.Generator())
    with pytest.raises(ValueError, match="drawn"):
        fused_mapper.update_model(None, [frame], frame, cfg, draw="device", drawn=torch.zeros((H, W), dtype=torch.bool))
    with pytest.raises(ValueError, match="'torch' or 'device'"):
        fused_mapper.update_model(None, [frame], frame, cfg, draw="philox")
    with pytest.raises(RuntimeError, match="ROCm device"):
        fused_mapper._densify_draw_device(cam, None, 0.5, 0.15, 0, 0)


def test_densify_model_takes_a_pixel_list_as_well_as_a_mask():
    """Golden G7's first keyframe on the CPU: the drawn pixels as the ascending int64 list the device draw returns append
    exactly the rows the (H,W) mask appends."""
    from types import SimpleNamespace
    from splat_loam_amd import fused_mapper
    from splat_loam_amd.scene import Camera, SurfelModel
    g = np.load(os.path.join(ROOT, "tests", "golden", "g7_update_model.npz"))
    lrs = tuple(float(v) for v in g["lr"])

    def brute_force_dist2(points):
        p = points.detach().double()
        d2 = torch.cdist(p, p) ** 2
        d2.fill_diagonal_(float("inf"))
        return d2.topk(3, dim=1, largest=False).values.mean(dim=1).float()
    rows = []
    drawn = torch.from_numpy(g["drawn_k0"])
    for form in (drawn, drawn.reshape(-1).nonzero().reshape(-1)):
        empty = lambda w: np.zeros((0, w), np.float32)
        model = SurfelModel(empty(3), empty(2), empty(4), empty(1), device="cpu")
        model.training_setup(*lrs, fused=False)
        cam = Camera(g["K"], g["depth_k0"], g["normal_k0"], g["valid_k0"], g["pose_k0"], data_device="cpu")
        frame = SimpleNamespace(camera=cam, model_T_frame=torch.tensor(g["pose_k0"]))
        n = fused_mapper.densify_model(model, frame, form, float(g["cfg"][5]), knn=brute_force_dist2)
        assert n == int(drawn.sum()) > 0
        rows.append([getattr(model, a).detach().clone() for a in ("_xyz", "_opacity", "_scaling", "_rotation")])
    for a, b in zip(*rows):
        assert torch.equal(a, b)
