"""The keyframe-batched step's C-ABI without a GPU: the per-keyframe struct's layout, the argument errors (returned
before anything is enqueued) and the workspace size."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from splat_loam_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 1000, 64, 1024


def test_keyframe_inputs_have_the_headers_layout(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    cls = _abi.SlsKeyframeInputs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sls_abi.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(SlsKeyframeInputs));',
             '  printf("max %d\\n", SLS_MAX_BATCH);']
    for field, _ in cls._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(SlsKeyframeInputs, {field}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((l.split()[0], int(l.split()[1])) for l in subprocess.check_output([str(exe)], text=True).splitlines() if l)
    assert got["size"] == C.sizeof(cls)
    assert got["max"] == _abi.SLS_MAX_BATCH == 8
    for field, _ in cls._fields_:
        assert got[field] == getattr(cls, field).offset, field


def _keyframes(G):
    """G keyframes whose buffers are distinct fake device addresses: the checks must reject the call before any of
    them is touched."""
    kfs = (_abi.SlsKeyframeInputs * G)()
    for g in range(G):
        k = kfs[g]
        k.cam.H, k.cam.W = H, W
        base = 0x10000000 * (g + 1)
        k.gt_depth, k.valid, k.col_cs, k.row_cs = base, base + 0x100000, base + 0x200000, base + 0x300000
        k.col_cs_half, k.row_cs_half, k.depth_order = base + 0x400000, base + 0x500000, base + 0x600000
        k.block_order, k.det_prev = base + 0x700000, base + 0x800000
        k.n_valid = 100
    return kfs


def _call(G, kfs):
    lib = _abi.lib()
    cfg = _abi.SlsMappingConfig()
    cfg.apply_adam = 1
    fake = 0x7F0000000000
    # (workspace_bytes = 0: should an argument check ever go missing, the call stops at the workspace size check,
    #  SLS_E_SCRATCH, before anything is enqueued on the fake addresses)
    return lib.sls_mapping_step_batch(G, kfs, N, *([fake] * 7), 1, C.byref(cfg), 1 << 20, fake, 0, fake, None)


def _expect_arg_error(G, kfs, words):
    rc = _call(G, kfs)
    assert rc == -1, rc              # SLS_E_ARG
    msg = _abi.lib().sls_last_error().decode()
    assert words in msg, msg


def test_argument_errors_return_sls_e_arg_before_any_launch():
    for G in (0, 9, -1):
        _expect_arg_error(G, _keyframes(max(G, 1)), "G: 1 to SLS_MAX_BATCH")
    kfs = _keyframes(3)
    kfs[2].cam.W = 2048
    _expect_arg_error(3, kfs, "one image size")
    kfs = _keyframes(3)
    kfs[1].cam.H = 32
    _expect_arg_error(3, kfs, "one image size")
    for field in ("gt_depth", "valid", "col_cs", "row_cs", "col_cs_half", "row_cs_half", "depth_order"):
        kfs = _keyframes(4)
        setattr(kfs[3], field, None)
        _expect_arg_error(4, kfs, "null per-keyframe pointer")
    kfs = _keyframes(4)
    kfs[2].depth_order = kfs[0].depth_order
    _expect_arg_error(4, kfs, "share one depth_order")
    kfs = _keyframes(4)
    kfs[3].block_order = kfs[1].block_order
    _expect_arg_error(4, kfs, "share one block_order")
    kfs = _keyframes(4)
    kfs[3].det_prev = kfs[1].det_prev
    _expect_arg_error(4, kfs, "share one det_prev")
    kfs = _keyframes(2)
    kfs[1].block_order = None
    _expect_arg_error(2, kfs, "block_order on every keyframe or on none")
    _expect_arg_error(1, None, "null pointer")
    # the shared configuration: a batch is one whole step on the flat bucket
    lib, fake = _abi.lib(), 0x7F0000000000
    for field, value in (("phase", 1), ("grad_chunk", 64), ("grad_bitmap", fake), ("union_bitmap", fake)):
        cfg = _abi.SlsMappingConfig()
        setattr(cfg, field, value)
        rc = lib.sls_mapping_step_batch(2, _keyframes(2), N, *([fake] * 7), 1, C.byref(cfg), 1 << 20, fake, 0,
                                        fake, None)
        assert rc == -1 and "one whole step" in lib.sls_last_error().decode(), field


def test_batch_workspace_grows_linearly_in_g():
    """One whole workspace (the scratch the keyframes' fronts share) + a per-keyframe part per further keyframe, which
    holds only what the batched projection backward reads: far smaller than a workspace of its own."""
    lib = _abi.lib()
    for det in (0, 1):
        cfg = _abi.SlsMappingConfig()
        cfg.deterministic = det
        one = lib.sls_mapping_workspace_bytes_cfg(N, H, W, 1 << 20, C.byref(cfg))
        assert one > 0
        assert lib.sls_mapping_workspace_bytes_batch(1, N, H, W, 1 << 20, C.byref(cfg)) == one
        part = lib.sls_mapping_workspace_bytes_batch(2, N, H, W, 1 << 20, C.byref(cfg)) - one
        assert 0 < part < one // 2
        for G in range(1, 9):
            assert lib.sls_mapping_workspace_bytes_batch(G, N, H, W, 1 << 20, C.byref(cfg)) == one + (G - 1) * part
        # the per-keyframe part does not depend on the instance capacity
        assert lib.sls_mapping_workspace_bytes_batch(2, N, H, W, 1 << 22, C.byref(cfg)) - \
            lib.sls_mapping_workspace_bytes_batch(1, N, H, W, 1 << 22, C.byref(cfg)) == part
        assert lib.sls_mapping_workspace_bytes_batch(0, N, H, W, 1 << 20, C.byref(cfg)) == 0
        assert lib.sls_mapping_workspace_bytes_batch(9, N, H, W, 1 << 20, C.byref(cfg)) == 0
