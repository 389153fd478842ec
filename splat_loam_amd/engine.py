"""MappingEngine: one native call per mapping iteration.

`Mapper.optimize` (slam/mapper.py:150-204) spends its time in ~120 small torch
kernels, a dozen allocations and several device->host syncs per iteration around
the rasterizer.  The engine keeps the model's four raw parameter tensors where
they are (torch Parameters), owns the flat gradient / Adam-state buckets and one
workspace, and issues `sls_mapping_step` — activations, rasterizer forward,
loss, backward, regulariser and Adam enqueued back to back on the stream with no
host sync; the iteration's status (instance count, overflow flag, loss terms) is
read once at the end, which is the same single sync per iteration the reference
has (`loss_total.item()`, slam/mapper.py:206-209).

Keyframe-parallel mode: every rank calls step() on ITS keyframe
with the same replicated model.  Two exchange schemes (`dp_mode`):
  "rs_ag" (default, even N): the gradients leave the native step in G chunks, a
      reduce-scatter gives every rank the summed chunk it owns, the rank applies
      Adam to THAT 1/G of the parameters (its Adam moments are the only ones it
      keeps: optimiser state sharded G ways), an all-gather republishes the
      parameters — the bytes of one all-reduce, the optimiser pass divided by G,
      replicas identical by construction;
  "allreduce": the flat 10*N bucket (+2 void words) is all-reduced in one RCCL
      collective and every rank applies the same guarded Adam update;
  "sparse" (even N): only the TOUCHED set travels (a keyframe reaches ~10 % of the
      surfels).  Behind the tile backward every rank knows which surfels CAN have a
      gradient (reached by its keyframe, or pushed by the scale regulariser): these
      bitmaps are all-gathered (N/8 bytes each) and OR-ed (sls_grad_union); the
      projection's backward then writes the union's 40-byte rows straight into their
      slots of the collective's buffer and applies Adam to every surfel OUTSIDE the
      union right there (zero gradient on every rank: the one-GPU update); the rows
      are SUM-reduced and sls_adam_step_sparse(part 2) updates the union.  No flat
      bucket, no packing launch, no second pass over the whole model.  The
      collective's size is a host-side capacity that follows the union's measured
      size; a union larger than it voids the iteration on every rank (bit 2 of the
      status word) and it is repeated with more room.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np
import torch
import torch.distributed as dist

from . import _abi
from .fused import camera_aux
from .rasterizer import GaussianRasterizationSettings, deterministic_mode, get_camera

# word 1 of the status block: any bit set = the iteration is void (Adam was skipped) and must be repeated
TOO_SMALL = 1               # the instance buffers were too small (word 0 = the room asked for)
RESORT_FAILED = 2           # the repaired depth order was not exact
EXCHANGE_TOO_SMALL = 4      # sparse exchange: the union of the touched sets outgrew the collective
DET_MISPREDICTED = 8        # deterministic = 2: a predicted fixed-point scale was too small
HANDOVER_MISMATCH = 16      # the tile backward met a hand-over buffer of another forward
OUTSIDE_UNION = 32          # sparse exchange: a gradient outside the agreed union


def status_dict(w, f):
    """The status dict from the block's eight words as Python ints (`w`) and as the floats the same bits spell (`f`)."""
    flags = w[1]
    return {"R": w[0] & 0xFFFFFFFF, "overflow": bool(flags), "too_small": bool(flags & TOO_SMALL),
            "resort_failed": bool(flags & RESORT_FAILED), "exchange_too_small": bool(flags & EXCHANGE_TOO_SMALL),
            "det_mispredicted": bool(flags & DET_MISPREDICTED), "handover_mismatch": bool(flags & HANDOVER_MISMATCH),
            "outside_union": bool(flags & OUTSIDE_UNION), "exchange_count": w[7] & 0xFFFFFFFF,
            "loss_pixel": f[5], "loss_reg": f[6], "loss": f[5] + f[6], "sums": [f[2], f[3], f[4]]}


def repair_rounds(age, base_rounds, max_order_age, order_age_round3, max_order_age_extra, order_age_round4, allow):
    """How a depth order last written `age` iterations ago (None: never) is brought up to date: 0 = from scratch,
    1..4 = that many repair rounds — `base_rounds`, one more beyond each of `max_order_age`, `order_age_round3` and
    `order_age_round4` (the surfels have drifted further), four at the most; an order older than
    `max_order_age_extra` is rebuilt, and so is every order where reuse is not allowed."""
    if not allow or age is None or age > max_order_age_extra:
        return 0
    return min(base_rounds + (age > max_order_age) + (age > order_age_round3) + (age > order_age_round4), 4)


class _Keyframe:
    """What the engine keeps per keyframe: its depth order and the iteration that wrote it (None: void), a weak
    reference to the camera (an id can be reused by a new object once the old keyframe is gone), the tile backward's
    launch order (SlsMappingConfig.block_order; zeros: none yet) and, under deterministic = 2 only, the uint8 (N, 16)
    predicted scales (None: nothing to predict from yet — the visit runs the two-launch scheme)."""
    __slots__ = ("order", "stamp", "camera", "block_order", "det_prev")

    def __init__(self, order, camera, block_order):
        self.order, self.stamp, self.camera, self.block_order, self.det_prev = order, None, weakref.ref(camera), block_order, None


def carry_bucket(buf: torch.Tensor, keep: torch.Tensor, n_new: int) -> torch.Tensor:
    """A flat 10*N_old bucket [xyz 3N | opacity N | scaling 2N | rotation 4N] -> the 10*n_new bucket of the surfel
    set that keeps the rows marked in `keep` (in order) and appends n_new - keep.sum() zero rows per group."""
    n_old = int(keep.numel())
    n_keep = int(keep.sum().item())
    if buf.numel() != 10 * n_old or n_new < n_keep:
        raise ValueError("bucket / mask / new size do not fit together")
    out = torch.zeros((10 * n_new,), dtype=buf.dtype, device=buf.device)
    src_off = dst_off = 0
    for width in (3, 1, 2, 4):
        src = buf[src_off:src_off + width * n_old].view(n_old, width)
        out[dst_off:dst_off + width * n_keep].view(n_keep, width).copy_(src[keep])
        src_off += width * n_old
        dst_off += width * n_new
    return out


def dp_chunk(N: int, G: int) -> int:
    """Elements per rank of the reduce-scatter layout: a multiple of 4 floats with G * C >= 10 N."""
    return -(-(10 * N) // (4 * G)) * 4


def dp_pieces(N: int, lo: int, hi: int, lrs):
    """The flat range [lo, hi) of [xyz 3N | opacity N | scaling 2N | rotation 4N] cut at the parameter-group
    boundaries: [(start, stop, learning rate)], at most four pieces."""
    out = []
    for g0, g1, lr in ((0, 3 * N, lrs[0]), (3 * N, 4 * N, lrs[1]), (4 * N, 6 * N, lrs[2]), (6 * N, 10 * N, lrs[3])):
        a, b = max(lo, g0), min(hi, g1)
        if b > a:
            out.append((a, b, lr))
    return out


def dp_chunked(flat: torch.Tensor, C: int, G: int) -> torch.Tensor:
    """Flat bucket -> the physical reduce-scatter layout (element e at e + 4 * (e // C); 4 spare words per chunk,
    the first two of which carry the void flags).  The native step writes this layout directly; this helper is
    the layout's definition in torch (tests, CPU emulation)."""
    out = torch.zeros((G, C + 4), dtype=flat.dtype, device=flat.device)
    pad = torch.zeros((G * C,), dtype=flat.dtype, device=flat.device)
    pad[:flat.numel()] = flat
    out[:, :C] = pad.view(G, C)
    return out.reshape(-1)


class MappingEngine:
    def __init__(self, model, cfg, lrs=(5e-4, 5e-2, 5e-3, 1e-3), betas=(0.9, 0.999), eps=1e-15,
                 capacity_factor: float = 1.3):
        self.model, self.cfg = model, cfg
        self.lrs, self.betas, self.eps = tuple(lrs), tuple(betas), float(eps)
        self.capacity_factor = float(capacity_factor)
        p = model._xyz
        if not p.is_cuda:
            raise RuntimeError("MappingEngine needs ROCm device parameters; there is no CPU fallback")
        self.dev = p.device
        self.N = int(p.shape[0])
        n10 = 10 * self.N
        # flat buckets; two extra words at the end of grads carry the two "iteration void" flags
        # (instance buffers too small, depth-order repair failed) through the all-reduce
        self.grads = torch.zeros((n10 + 2,), dtype=torch.float32, device=self.dev)
        self.exp_avg = torch.zeros((n10,), dtype=torch.float32, device=self.dev)
        self.exp_avg_sq = torch.zeros((n10,), dtype=torch.float32, device=self.dev)
        self.status = torch.zeros((8,), dtype=torch.int32, device=self.dev)
        self.t = 0
        self.capacity = 0
        self.workspace = None
        self._ws_n = 0                    # surfels the workspace was sized for
        self._bucket_store = None         # resize(): the three flat buckets' backing store, with head room
        self._bws = None                  # step_batch()'s workspace (_ensure_batch_workspace)
        self.last_batch_reuse = None      # repair rounds of the last batch's keyframes
        self.allmap_ptr = C.c_void_p(0)
        self.last = None
        # lagged status read (sync="lagged"): two status slots on the device, pinned mirrors, events
        self._lag_dev = torch.zeros((2, 8), dtype=torch.int32, device=self.dev)
        self._lag_host = torch.zeros((2, 8), dtype=torch.int32).pin_memory()
        self._lag_ev = [torch.cuda.Event(), torch.cuda.Event()]
        # With the status mirror (the iteration's last kernel stores the status block into pinned host memory, word 7
        # last) the host needs no event to know that an iteration has finished: it arms words 0 and 7 of the slot with a
        # value the device never writes and polls them — no event record on the stream, no event wait
        # (status_poll = False: events; kept as an attribute for the equality tests, its verdict is in HISTORY.md)
        self._lag_np = self._lag_host.numpy()
        self.status_poll = True
        self._lag_polled = [False, False]
        self._group = None
        self._lag_ready = []              # statuses of finished iterations not handed out yet (lagged mode)
        self.flushed = []
        self._lag_pending = None          # (slot, camera) of the iteration whose status was not read yet
        # temporal re-sort: the workspace keeps the depth order of the last iteration; it is repaired
        # instead of recomputed when the next iteration renders the same keyframe (reuse_depth_order)
        self.reuse_depth_order = True
        # the loss stage inside the tile backward (no launch of its own; the backward's launch order then comes from the
        # keyframe's previous iteration): same gradients bit for bit
        self.inline_loss_stage = True
        self.repair_span = 256            # iterations an extra repair round stays on after a repair that did not reach
        self._repair_rounds, self._repair_until = 1, 0
        # single GPU: Adam is applied inside the backward; the flat gradient bucket is only filled when asked
        # for (the reference drops its gradients right after optimizer.step() as well)
        self.keep_grads = False
        self._ws_ready = False
        self._ws_hw = None
        self._ws_det = None
        self.status_mirror = True          # (False: the status through a device -> host copy; lagged mode)
        # one cache entry per keyframe (the mapper samples keyframes at random, slam/mapper.py:152-156):
        # id(camera) -> _Keyframe, at most max_cached_orders of them, oldest first out; an order older than
        # max_order_age iterations gets an extra repair round, one older than max_order_age_extra is rebuilt
        self._orders = {}
        self._set_order_ages()
        self.max_cached_orders = 64
        self.stats = {"repeated_too_small": 0, "repeated_resort": 0, "repeated_exchange": 0, "repeated_det": 0}
        self._enq = 0                     # iterations enqueued so far (age of the cached depth orders)
        # keyframe-parallel exchange (set up at the first sharded step)
        self.dp_mode = os.environ.get("SLS_DP_MODE", "rs_ag")
        self._dp = None                   # dict(G, rank, C, flat, gshard) once the reduce-scatter layout is in place
        self._dp_agreed, self._dp_use_rs, self._dp_scheme = None, False, 0    # (G, rank) the scheme was agreed for; the agreed verdict
        # integer-atomic gradient accumulation: False / True (SLS_DETERMINISTIC=1: two tile-backward launches) / 2
        # (SLS_DETERMINISTIC=2: one launch with scales predicted from the keyframe's previous iteration; the first
        # iteration on a workspace, and any iteration after a misprediction, run the two-launch scheme)
        self.deterministic = 2 if os.environ.get("SLS_DETERMINISTIC", "0") == "2" else deterministic_mode()
        self._det_two_pass_next = True    # the next deterministic iteration runs the two-launch scheme
        self.block_masks = int(os.environ.get("SLS_BLOCK_MASKS", "0"))   # 0: auto (long lists), 1: always, 2: never (SlsMappingConfig.block_masks)
        self._sx = None                   # sparse exchange: dict(bitmap, prefix, compact, cap, send) once set up
        self.exchanged_bytes = 0          # bytes this rank handed to collectives in the last keyframe-parallel step
        self.exchange_at_world_1 = False  # take the keyframe-parallel path (collectives + separate Adam) in a 1-rank group too
        self.comm_events = None           # list -> (start, after exchange, after Adam[, after all-gather]) events per step
        self._last_call = None            # (arguments, config) of the last sls_mapping_step: phase 2 repeats them
        # pose gradient: dL/dxi of the pixel loss for the left perturbation of the keyframe's
        # view transform — (6,) [v | w] after step(..., pose_grad=True) / pose_step(), (G, 6) after step_batch(...,
        # pose_grad=True); views of one device buffer, valid until the next such call
        self.pose_grad = None
        self._pose_buf = torch.zeros((_abi.SLS_MAX_BATCH, 6), dtype=torch.float32, device=self.dev)
        self._pose_scratch = None

    # views of the flat gradient bucket in the optimiser's group order (single GPU: only filled
    # when keep_grads is set; keyframe-parallel mode always fills and all-reduces it)
    def grad_views(self):
        N = self.N
        g = self.grads
        if self._dp is not None:          # reduce-scatter layout -> flat copy (diagnostics / tests only)
            C, G = self._dp["C"], self._dp["G"]
            g = g.view(G, C + 4)[:, :C].reshape(-1)[:10 * N].clone()
        return {"xyz": g[0:3 * N].view(N, 3), "opacity": g[3 * N:4 * N].view(N, 1),
                "scaling": g[4 * N:6 * N].view(N, 2), "rotation": g[6 * N:10 * N].view(N, 4)}

    def _ensure_workspace(self, H, W, capacity):
        lib = _abi.lib()
        if (self.workspace is None or capacity > self.capacity or (H, W) != self._ws_hw
                or self._ws_det != bool(self.deterministic) or self.N > self._ws_n):
            self._ws_det = bool(self.deterministic)
            self.capacity, self._ws_hw = int(max(capacity, self.capacity)), (H, W)   # (keyframes of another size: re-carve)
            wcfg = _abi.SlsMappingConfig()
            wcfg.deterministic = 1 if self.deterministic else 0     # (the fixed-point accumulators only when asked for)
            # (sized for a quarter more surfels than there are: resize() keeps it while the model grows into that room)
            self._ws_n = self.N + (self.N // 4 if self._bucket_store is not None else 0)
            nbytes = int(lib.sls_mapping_workspace_bytes_cfg(self._ws_n, H, W, self.capacity, C.byref(wcfg)))
            self.workspace = None     # release before re-allocating
            self.workspace = torch.empty((nbytes + 256,), dtype=torch.uint8, device=self.dev)
            self._ws_ready = False
        return self._aligned(self.workspace)

    @staticmethod
    def _aligned(buf):
        """(pointer, bytes) of a workspace buffer allocated with 256 bytes to spare: its first 256-byte boundary on."""
        return (buf.data_ptr() + 255) & ~255, buf.numel() - 256

    def _first_capacity(self):
        if self.capacity == 0:
            self.capacity = max(4 * self.N, 1 << 16)
        return self.capacity

    def _config(self, apply_adam, with_regulariser, reuse_order=False):
        c, cfg = _abi.SlsMappingConfig(), self.cfg
        c.reuse_depth_order = int(reuse_order)      # 0: from scratch, 1 / 2: repair with that many rounds
        c.keep_grads = 1 if self.keep_grads else 0
        c.workspace_ready = 1 if self._ws_ready else 0
        self._ws_ready = True
        c.lambda_alpha, c.lambda_normal = cfg.opt_lambda_alpha, cfg.opt_lambda_normal
        c.scaling_max = cfg.opt_scaling_max
        c.scaling_max_penalty = cfg.opt_scaling_max_penalty if with_regulariser else 0.0
        c.depth_ratio = cfg.depth_ratio
        c.lr_xyz, c.lr_opacity, c.lr_scaling, c.lr_rotation = self.lrs
        c.apply_adam = 1 if apply_adam else 0
        c.beta1, c.beta2, c.eps = self.betas[0], self.betas[1], self.eps
        if self._dp is not None and not apply_adam:
            c.grad_chunk, c.grad_ranks = self._dp["C"], self._dp["G"]
        c.deterministic = 1 if self.deterministic else 0      # (_enqueue raises it to 2 where the one-launch scheme applies)
        c.block_masks = int(self.block_masks)
        if self._sx is not None and not apply_adam:
            c.grad_bitmap = self._sx["mine"].data_ptr()
        return c

    def _order_entry(self, camera):
        ent = self._orders.get(id(camera))
        return ent if ent is not None and ent.camera() is camera else None

    def _forget_order(self, camera, failed_repair=False):
        ent = self._order_entry(camera)
        if ent is not None:
            ent.stamp = None
        if failed_repair:
            self._repair_rounds = min(self._repair_rounds + 1, 3)
            self._repair_until = self._enq + self.repair_span

    def _set_order_ages(self):
        """The ages (iterations since the keyframe was last rendered) that decide how a keyframe's depth order is
        brought up to date: one repair round up to `max_order_age`, two up to `order_age_round3`, three up to
        `max_order_age_extra` (four beyond `order_age_round4`), a rebuild beyond.  A round reaches 512 POSITIONS, and
        how many positions a surfel travels for the same change of depth grows with the number of surfels: measured
        at 500 k surfels (4 / 12 / 48; looser values fail repairs, each costs a void iteration + a rebuild) and at
        170 k / 50 k (12 / 32 / 200 without a failure, -1.5 % / -2.5 % per iteration with the mapper's keyframe
        sampling), hence the scale with 500 k / N, capped at 3.  Further repair rounds run inside the one merge launch, where a window needs
        them: under 1 us where it turns out that none does, 8-20 us where many do; the radix sort costs 90.
        (The four ages are plain attributes; what other values cost is in HISTORY.md #44, #50, #51.)"""
        scale = min(max(500000.0 / max(self.N, 1), 1.0), 3.0)
        self.max_order_age = int(4 * scale)
        self.order_age_round3 = int(12 * scale)
        self.max_order_age_extra = int(48 * scale)
        self.order_age_round4 = 1000000

    def _keyframe_inputs(self, camera, H, W, allow_reuse, advance=True):
        """What one keyframe hands to the native step: its camera entry, its aux tables, its cache entry (created on
        the first visit) and how the iteration enqueued next brings its depth order up to date (repair_rounds).
        advance=False: the caller counts the iteration and stamps the entry itself (a batch is ONE update)."""
        ce = get_camera(GaussianRasterizationSettings(H, W, 1.0, camera.world_view_transform, camera.projection_matrix),
                        self.dev)
        aux = camera_aux(camera)
        ent = self._order_entry(camera)
        if ent is None:
            for k in [k for k, e in self._orders.items() if e.camera() is None]:
                del self._orders[k]
            # (an evicted keyframe's next visit sorts from scratch and, under deterministic = 2, takes two launches,
            #  as a first visit does; the predicted scales alone are 16 N bytes per keyframe)
            while len(self._orders) >= self.max_cached_orders:
                self._orders.pop(next(iter(self._orders)))
            ent = self._orders[id(camera)] = _Keyframe(
                torch.empty((self.N,), dtype=torch.int32, device=self.dev), camera,
                torch.zeros((int(_abi.lib().sls_block_order_bytes(H, W)) // 4,), dtype=torch.int32, device=self.dev))
        # after a failed repair the following iterations repair with one more round (one more window of reach,
        # still one launch: HISTORY.md #83); every `repair_span` iterations without a failure the number of rounds steps down again
        if self._repair_rounds > 1 and self._enq >= self._repair_until:
            self._repair_rounds -= 1
            self._repair_until = self._enq + self.repair_span
        reuse = repair_rounds(None if ent.stamp is None else self._enq - ent.stamp, self._repair_rounds,
                              self.max_order_age, self.order_age_round3, self.max_order_age_extra,
                              self.order_age_round4, allow_reuse and self.reuse_depth_order)
        if advance:
            self._enq += 1
            ent.stamp = self._enq
        return ce, aux, ent, reuse

    def _det_prev_ptr(self, ent):
        """The keyframe's predicted scales (deterministic = 2), allocated where it has none yet."""
        if ent.det_prev is None:
            ent.det_prev = torch.zeros((self.N, 16), dtype=torch.uint8, device=self.dev)
        return ent.det_prev.data_ptr()

    def _pose_args(self, cfg, slots):
        """The pose gradient's scratch (zeroed once; every call leaves it ready) into `cfg`."""
        need = int(_abi.lib().sls_pose_grad_scratch_bytes(self.N)) * int(slots)
        if self._pose_scratch is None or self._pose_scratch.numel() < need:
            self._pose_scratch = torch.zeros((need,), dtype=torch.uint8, device=self.dev)
        cfg.pose_scratch, cfg.pose_scratch_bytes = self._pose_scratch.data_ptr(), int(self._pose_scratch.numel())

    def _params(self):
        m = self.model
        ps = (m._xyz, m._scaling, m._rotation, m._opacity)
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.shape[0] != self.N:
                raise RuntimeError("model parameters must stay contiguous float32 of the engine's size")
        return ps

    def _enqueue(self, camera, apply_adam, with_regulariser, status=None, mirror=None, allow_reuse=True, phase=0,
                 pose_grad=False):
        lib = _abi.lib()
        H, W = int(camera.image_height), int(camera.image_width)
        ws_ptr, ws_bytes = self._ensure_workspace(H, W, self._first_capacity())
        xyz, scaling, rotation, opacity = self._params()
        ce, aux, ent, reuse = self._keyframe_inputs(camera, H, W, allow_reuse)
        cfg = self._config(apply_adam, with_regulariser, reuse)
        if self.deterministic == 2:
            first_visit = ent.det_prev is None
            cfg.det_prev = self._det_prev_ptr(ent)
            # two launches where there is nothing to predict from: a workspace's first deterministic iteration (it sets
            # the fields' default scales) and a keyframe's first visit (measured: predicting a new view from the
            # defaults alone voids the iteration almost every time)
            cfg.deterministic = 1 if (self._det_two_pass_next or first_visit or not cfg.workspace_ready) else 2
            self._det_two_pass_next = False
        cfg.depth_order = ent.order.data_ptr()
        cfg.block_order = ent.block_order.data_ptr() if self.inline_loss_stage else None
        cfg.status_mirror = mirror
        # keyframe-parallel mode: the void bits leave the step as two floats behind the gradient bucket
        cfg.void_flags_out = None if (apply_adam or self._dp is not None) else self.grads.data_ptr() + 4 * 10 * self.N
        cfg.phase = int(phase)
        if pose_grad:
            cfg.pose_grad = self._pose_buf.data_ptr()
            self._pose_args(cfg, 1)
        args = (C.byref(ce.cam), self.N, xyz.data_ptr(), scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(),
                self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.t + 1,
                aux.gt.data_ptr(), aux.valid.data_ptr(), aux.n_valid, ce.col_cs.data_ptr(), ce.row_cs.data_ptr(),
                aux.col_h.data_ptr(), aux.row_h.data_ptr(), C.byref(cfg), self.capacity, ws_ptr, ws_bytes,
                (self.status if status is None else status).data_ptr(), C.byref(self.allmap_ptr),
                torch.cuda.current_stream(self.dev).cuda_stream)
        self._last_call = (args, cfg) if phase == 1 else None      # (cfg and the camera entry stay alive with it)
        _abi.check(lib.sls_mapping_step(*args), "sls_mapping_step")

    @staticmethod
    def _void_reason(st):
        if st["too_small"]:
            return "repeated_too_small"
        if st["resort_failed"]:
            return "repeated_resort"
        return "repeated_det" if st.get("det_mispredicted") else "repeated_exchange"

    def _grown(self, need):
        """The instance capacity after an iteration that asked for `need` instances found too little room."""
        return int(max(need, self.capacity) * self.capacity_factor) + 1024

    def _after_void(self, voided, sharded, verdict=None):
        """Everything that follows a void status, before the repeat.  `voided`: (camera, status) of every iteration —
        or keyframe of a batch — the repeat covers; `verdict`: a batch's own status, which then decides in their place.
        Each void keyframe's depth order is forgotten where it may be broken or was never written (a failed repair
        raises the repair rounds), stats counts ONE repeat under the reason of the verdict (else of the first status),
        and if room was what lacked, capacity grows from the largest R and both workspaces are dropped (re-carved at
        the next enqueue; the batch's would be anyway: any change of capacity re-carves it).
        What the four callers keep to themselves, on purpose:
          step()         sharded, the status bits are the group's verdict and R is this rank's: MAX over the ranks;
          step_batch()   voided = the keyframes with their own statuses (this rank's), verdict = the batch's (R their
                         maximum, bits their OR; sharded as in step());
          pose_step()    never sharded; touches neither t nor last;
          _lag_collect() voided = the one or two in-flight iterations; sharded=False even over a group (no collective
                         there: a rank grows from the R it saw, the redo goes through step()); its own bookkeeping of t.
        The MAX all-reduce is issued exactly when `sharded` and the deciding status says too_small: that status is
        the group's verdict there, identical on every rank, so every rank issues the same collectives."""
        for camera, st in voided:
            if st["too_small"] or st["resort_failed"]:
                self._forget_order(camera, failed_repair=st["resort_failed"])
        deciding = [st for _, st in voided] if verdict is None else [verdict]
        self.stats[self._void_reason(deciding[0])] += 1
        if any(st["too_small"] for st in deciding):
            need = max(st["R"] for st in deciding)
            if sharded:
                t = torch.tensor([need], dtype=torch.int64, device=self.dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self._group)
                need = int(t.item())
            self.capacity = self._grown(need)
            self.workspace = self._bws = None

    def _sharded(self, group):
        """Keyframe-parallel path?  World size > 1 — or 1 with `exchange_at_world_1` (the collectives then move
        a rank's data onto itself: how the RCCL path is exercised on a one-GPU box)."""
        if not dist.is_initialized():
            return False
        return dist.get_world_size(group) > 1 or self.exchange_at_world_1

    def _read_status(self):
        return self._note(self._parse_status(self.status.cpu()))   # the one sync of the iteration

    def _note(self, st):
        """Host-side bookkeeping driven by a status every rank sees identically: the sparse exchange's collective
        size follows the measured size of the union of the touched sets: up at once (50 % + 4096 slots of head room
        — keyframes of a window reach sets of different size, and an iteration voided by a union that outgrew the
        collective costs more than a few hundred KB on the wire), down by 3 % per iteration."""
        # One-launch deterministic mode: the repeat of ANY voided iteration runs the two-launch scheme.  A misprediction
        # (bit 3) is what calls for it, but the keyframe-parallel verdicts fold every bit above bit 0 into bit 1 on their
        # way through the collectives, so the host cannot tell it from a failed repair there — and a one-launch repeat
        # with the same parameters and the same predictions would mispredict again, for ever.
        if st["overflow"] and self.deterministic == 2:
            self._det_two_pass_next = True            # (and with it the defaults' refresh)
        if st.get("outside_union"):
            raise RuntimeError("a surfel outside the agreed union of the touched sets had a non-zero gradient: the early "
                               "gradient bitmap was no superset (sparse exchange) — the iteration's update is void")
        if st.get("handover_mismatch"):
            raise RuntimeError("the tile backward found a forward -> backward hand-over buffer that is not this forward's "
                               "(its tag word does not match): the iteration's gradients are void")
        if self._sx is not None and (not st["overflow"] or st["exchange_too_small"]):
            want = int(st["exchange_count"] * 1.5) + 4096
            self._sx["send"] = int(min(self.N, max(want, int(self._sx["send"] * 0.97))))
        return st

    @staticmethod
    def _parse_status(h):
        return status_dict(h.tolist(), h.view(torch.float32).tolist())

    @staticmethod
    def _parse_status_np(h):
        """_parse_status on a NumPy row (int32 x 8) of the pinned mirror: no tensor ops on the host's critical path"""
        return status_dict(h.tolist(), h.view(np.float32).tolist())

    @torch.no_grad()
    def step(self, camera, group=None, sync: bool = True, pose_grad: bool = False):
        """One mapping iteration on `camera`.  Returns the status dict (sync=True)
        or None (sync=False: fire-and-forget — nobody reads the status, so an iteration
        that overflowed its instance buffers is DROPPED, not repeated (its Adam update
        was skipped on the device, the model stays intact), and `self.t` counts enqueued
        iterations, which can then run ahead of the updates applied; use "lagged" when
        every iteration has to count).
        sync="lagged": the iteration is enqueued BEFORE the status of
        the previous one is read, so the GPU queue never runs dry while the host
        waits for a loss value; returns the PREVIOUS iteration's status (None on
        the first call) — finish with flush().
        pose_grad=True (sync=True, one process): the iteration also leaves dL/dxi of the keyframe's pixel loss in
        `self.pose_grad` ((6,) device tensor, [v | w]) — the gradient at the parameters the
        iteration STARTED from; valid when the returned status is not void (a void iteration is repeated, as ever).
        Over a process group it raises: nothing about the pose is exchanged between ranks, and that path is not covered."""
        sharded = self._sharded(group)
        if pose_grad:
            if sync is not True:
                raise ValueError("pose_grad needs sync=True: the gradient belongs to the iteration whose status is returned")
            if sharded:
                raise NotImplementedError("pose_grad is served on the single-process path only")
        if self._dp is not None and not sharded:
            raise RuntimeError("this engine's optimiser state is sharded over a process group (dp_mode rs_ag): "
                               "it cannot take a single-process step")
        self._group = group
        if sync == "lagged":
            return self._step_lagged(camera)
        if self._lag_pending is not None:
            self.flush()
        # Fire-and-forget iterations sort from scratch: nobody would notice a repair that did not reach, and every
        # later repair of that keyframe would start from the broken order and void its iteration as well.
        reuse_ok = sync is not False
        while True:
            if not sharded:
                self._enqueue(camera, apply_adam=True, with_regulariser=True, allow_reuse=reuse_ok, pose_grad=pose_grad)
            else:
                rank = dist.get_rank(group)
                self._ensure_dp(group)
                self._enqueue(camera, apply_adam=False, with_regulariser=(rank == 0), allow_reuse=reuse_ok,
                              phase=self._phase_for_exchange())
                # the step left its void flags behind the gradients: no torch glue kernels; any rank's flag voids
                # the iteration everywhere: Adam reads the reduced flags and stores the group's verdict into the
                # local status word, so the one status read below is the only sync
                self._exchange_and_adam(group, self.status, None)
            if not sync:
                self.t += 1
                return None
            st = self._read_status()
            if not st["overflow"]:
                self.t += 1
                self.last = st
                self.pose_grad = self._pose_buf[0] if pose_grad else None
                return st
            # repeat the iteration (parameters were not touched): with the full sort, and with more
            # room if the instance buffers were too small
            self._after_void([(camera, st)], sharded)

    @torch.no_grad()
    def pose_step(self, camera):
        """One iteration on `camera` with the MODEL FROZEN: forward, pixel loss, backward — no Adam, no scale regulariser;
        parameters, moments and the step count stay as they are.  Leaves dL/dxi in `self.pose_grad` ((6,), [v | w]) and
        returns the status dict (its "loss" is the pixel loss).  What a model-frozen pose refinement iterates
        (pose.refine_pose); a void iteration is repeated as step() repeats one."""
        if self._dp is not None or self._sx is not None:
            raise RuntimeError("this engine's gradient bucket is laid out for a keyframe-parallel exchange: pose_step "
                               "needs the single-process engine")
        if self._lag_pending is not None:
            self.flush()
        while True:
            self._enqueue(camera, apply_adam=False, with_regulariser=False, pose_grad=True)
            st = self._read_status()
            if not st["overflow"]:
                self.pose_grad = self._pose_buf[0]
                return st
            self._after_void([(camera, st)], sharded=False)

    def _ensure_batch_workspace(self, G, H, W, capacity):
        """The batch's workspace: one slice per keyframe, kept apart from step()'s (re-carved for more keyframes, another
        size, more room or another accumulation mode)."""
        lib = _abi.lib()
        b = self._bws
        det = bool(self.deterministic)
        # (capacity: the slices are laid out by it, so ANY change re-carves — a smaller one would move the zeroed records)
        if b is None or G > b["G"] or capacity != b["cap"] or (H, W) != b["hw"] or det != b["det"] or self.N != b["n"]:
            wcfg = _abi.SlsMappingConfig()
            wcfg.deterministic = 1 if det else 0
            Gw = max(G, b["G"] if b is not None and (H, W) == b["hw"] else 1)
            nbytes = int(lib.sls_mapping_workspace_bytes_batch(Gw, self.N, H, W, capacity, C.byref(wcfg)))
            self._bws = None
            b = self._bws = {"G": Gw, "cap": int(capacity), "hw": (H, W), "det": det, "n": self.N, "ready": 0,
                             "buf": torch.empty((nbytes + 256,), dtype=torch.uint8, device=self.dev),
                             "status": torch.zeros((_abi.SLS_MAX_BATCH + 1, 8), dtype=torch.int32, device=self.dev)}
        return (b,) + self._aligned(b["buf"])

    def _enqueue_batch(self, cameras, apply_adam, with_regulariser, allow_reuse=True, pose_grad=False):
        """sls_mapping_step_batch on `cameras` with the keyframes' own cached orders (as _enqueue)."""
        lib = _abi.lib()
        G = len(cameras)
        H, W = int(cameras[0].image_height), int(cameras[0].image_width)
        b, ws_ptr, ws_bytes = self._ensure_batch_workspace(G, H, W, self._first_capacity())
        xyz, scaling, rotation, opacity = self._params()
        kfs = (_abi.SlsKeyframeInputs * G)()
        # (an order's age counts parameter updates: the whole batch is one, so a keyframe batched at every step stays
        #  one update old; the camera tables in this list must outlive the call)
        inputs = [self._keyframe_inputs(camera, H, W, allow_reuse, advance=False) for camera in cameras]
        for g, (ce, aux, ent, reuse) in enumerate(inputs):
            k = kfs[g]
            k.cam = ce.cam
            k.gt_depth, k.valid, k.n_valid = aux.gt.data_ptr(), aux.valid.data_ptr(), aux.n_valid
            k.reuse_depth_order = reuse
            k.col_cs, k.row_cs = ce.col_cs.data_ptr(), ce.row_cs.data_ptr()
            k.col_cs_half, k.row_cs_half = aux.col_h.data_ptr(), aux.row_h.data_ptr()
            k.depth_order = ent.order.data_ptr()
            k.block_order = ent.block_order.data_ptr() if self.inline_loss_stage else None
            # (deterministic = 2 runs as 1 in a batch; the keyframe's predictions are still rewritten for its step())
            k.det_prev = self._det_prev_ptr(ent) if self.deterministic == 2 else None
            k.pose_grad = self._pose_buf[g].data_ptr() if pose_grad else None
        self._enq += 1
        for _, _, ent, _ in inputs:
            ent.stamp = self._enq
        ready = self._ws_ready
        cfg = self._config(apply_adam, with_regulariser)
        self._ws_ready = ready          # (that flag is step()'s workspace's)
        # the slices whose accumulation buffers are known to be zero (a first use zeroes the batch's G slices)
        cfg.workspace_ready = 1 if G <= b["ready"] else 0
        b["ready"] = max(b["ready"], G)
        cfg.void_flags_out = None if apply_adam else self.grads.data_ptr() + 4 * 10 * self.N
        if pose_grad:
            self._pose_args(cfg, G)
        self.last_batch_reuse = [reuse for _, _, _, reuse in inputs]
        _abi.check(lib.sls_mapping_step_batch(G, kfs, self.N, xyz.data_ptr(), scaling.data_ptr(), rotation.data_ptr(),
                                              opacity.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                              self.exp_avg_sq.data_ptr(), self.t + 1, C.byref(cfg), b["cap"],
                                              ws_ptr, ws_bytes, b["status"].data_ptr(),
                                              torch.cuda.current_stream(self.dev).cuda_stream),
                   "sls_mapping_step_batch")
        return b["status"]

    @torch.no_grad()
    def step_batch(self, cameras, group=None, sync: bool = True, pose_grad: bool = False):
        """ONE mapping iteration over up to eight distinct keyframes of the same size: the keyframes' pixel-loss gradients
        summed, the scale regulariser once, one Adam update (`self.t` + 1).  Returns the batch's status dict, with the
        keyframes' own statuses (R, bits, loss sums) under "keyframes" (sync=True), or None (sync=False, as step()).
        A void keyframe voids the batch; it is repeated as step() repeats an iteration.
        With `group` (dp_mode "allreduce"), every rank batches ITS keyframes and the summed gradient is all-reduced over
        the ranks before the guarded Adam: 8 keyframes on 2 or 4 GPUs; the regulariser counts on rank 0 only.
        pose_grad=True (sync=True, one process): `self.pose_grad` is (G, 6) afterwards, row g = dL_g/dxi of keyframe g's
        pixel loss through its own camera (as step()); what to do with the G gradients is the caller's."""
        cams = list(cameras)
        if pose_grad and sync is not True:
            raise ValueError("pose_grad needs sync=True: the gradients belong to the iteration whose status is returned")
        if pose_grad and self._sharded(group):
            raise NotImplementedError("pose_grad is served on the single-process path only")
        if sync == "lagged":
            raise ValueError("step_batch has no lagged mode")
        if not 1 <= len(cams) <= _abi.SLS_MAX_BATCH:
            raise ValueError(f"a batch holds 1 to {_abi.SLS_MAX_BATCH} keyframes, not {len(cams)}")
        if len({id(c) for c in cams}) != len(cams):
            raise ValueError("a keyframe appears twice in the batch")
        if len({(int(c.image_height), int(c.image_width)) for c in cams}) != 1:
            raise ValueError("the keyframes of a batch must share one image size")
        sharded = self._sharded(group)
        if sharded and self.dp_mode != "allreduce":
            raise NotImplementedError(f"step_batch over a process group needs dp_mode 'allreduce', not {self.dp_mode!r}")
        if self._dp is not None or self._sx is not None:
            raise RuntimeError("this engine's optimiser state is laid out for another exchange: step_batch cannot use it")
        self._group = group
        if self._lag_pending is not None:
            self.flush()
        reuse_ok = sync is not False
        while True:
            if not sharded:
                status = self._enqueue_batch(cams, apply_adam=True, with_regulariser=True, allow_reuse=reuse_ok,
                                             pose_grad=pose_grad)
            else:
                self._ensure_dp(group)
                status = self._enqueue_batch(cams, apply_adam=False, with_regulariser=(dist.get_rank(group) == 0),
                                             allow_reuse=reuse_ok)
                self._exchange_and_adam(group, status[0], None)
            if not sync:
                self.t += 1
                return None
            h = status[:len(cams) + 1].cpu()
            st = self._note(self._parse_status(h[0]))
            st["keyframes"] = [self._parse_status(h[1 + g]) for g in range(len(cams))]
            if not st["overflow"]:
                self.t += 1
                self.last = st
                self.pose_grad = self._pose_buf[:len(cams)] if pose_grad else None
                return st
            self._after_void(list(zip(cams, st["keyframes"])), sharded, verdict=st)

    def _step_lagged(self, camera):
        slot = 0 if self._lag_pending is None else self._lag_pending[0] ^ 1
        group = self._group
        polled = False
        if self._sharded(group):
            # keyframe-parallel: the group's verdict is known on the device only (the void flags ride the
            # gradient all-reduce and guard Adam), so the host can lag here exactly as on one GPU
            self._ensure_dp(group)
            self._enqueue(camera, apply_adam=False, with_regulariser=(dist.get_rank(group) == 0),
                          status=self._lag_dev[slot], phase=self._phase_for_exchange())
            self._exchange_and_adam(group, self._lag_dev[slot],
                                    self._lag_host[slot].data_ptr() if self.status_mirror else None)
            if not self.status_mirror:
                self._lag_host[slot].copy_(self._lag_dev[slot], non_blocking=True)
        elif self.status_mirror:
            # the iteration's last kernel mirrors the status block into pinned host memory: no copy kernel
            polled = self.status_poll
            if polled:
                self._lag_np[slot, 0] = -1
                self._lag_np[slot, 7] = -1
            self._enqueue(camera, apply_adam=True, with_regulariser=True, status=self._lag_dev[slot],
                          mirror=self._lag_host[slot].data_ptr())
        else:
            self._enqueue(camera, apply_adam=True, with_regulariser=True, status=self._lag_dev[slot])
            self._lag_host[slot].copy_(self._lag_dev[slot], non_blocking=True)
        self.t += 1
        self._lag_polled[slot] = polled
        if not polled:
            self._lag_ev[slot].record(torch.cuda.current_stream(self.dev))
        prev, self._lag_pending = self._lag_pending, (slot, camera)
        if prev is not None:
            self._lag_collect(prev, redo_current=True)
        # every iteration's status is handed out exactly once, oldest first (a repeated iteration makes two
        # of them available at once: the next call returns the second)
        return self._lag_ready.pop(0) if self._lag_ready else None

    def _lag_collect(self, prev, redo_current):
        pslot, pcam = prev
        if self._lag_polled[pslot]:
            row, spins = self._lag_np[pslot], 0
            while row[7] == -1 or row[0] == -1:          # (the device writes word 7 last, and never this value)
                spins += 1
                if spins > 2_000_000:                    # ~1 s: something else is wrong — let the stream say what
                    torch.cuda.current_stream(self.dev).synchronize()
                    if row[7] == -1 or row[0] == -1:
                        raise RuntimeError("the mapping iteration's status never reached its host mirror")
            st = self._note(self._parse_status_np(row.copy()))
        else:
            self._lag_ev[pslot].synchronize()
            st = self._note(self._parse_status(self._lag_host[pslot].clone()))
        if not st["overflow"]:
            self.last = st
            self._lag_ready.append(st)
            return st
        # The instance buffers were too small: that iteration skipped its Adam update on the
        # device, and so did the one enqueued after it (same capacity).  Drain, grow, redo.
        cur, self._lag_pending = self._lag_pending, None
        torch.cuda.current_stream(self.dev).synchronize()
        cur_st = self._note(self._parse_status(self._lag_dev[cur[0]].cpu())) if cur is not None else None
        cur_void = cur_st is not None and cur_st["overflow"]
        # both in-flight iterations are taken off the step count; the one that did run is put back after the
        # redo below, so that the repeated iteration uses the Adam step number it was meant to have
        self.t -= 2 if cur is not None else 1
        self._after_void([(pcam, st)] + ([(cur[1], cur_st)] if cur_void else []), sharded=False)
        if cur_st is not None and not cur_void:
            self._lag_ready.append(cur_st)   # (another keyframe that fitted: it did run, nothing to repeat)
        st = self.step(pcam, group=self._group, sync=True)
        self._lag_ready.append(st)
        if cur is not None and not cur_void:
            self.t += 1
        if cur_void:
            if redo_current:
                # (not through _step_lagged: its return value would take a status off the queue)
                self._redo_pending(cur[1])
            else:
                self._lag_ready.append(self.step(cur[1], group=self._group, sync=True))
        return st

    def _redo_pending(self, camera):
        ready, self._lag_ready = self._lag_ready, []
        self._step_lagged(camera)                    # enqueues it again; nothing older is pending
        self._lag_ready = ready + self._lag_ready

    def flush(self):
        """Drains the lagged pipeline: returns the status of the LAST iteration (None if there was none);
        `self.flushed` lists every status that had not been handed out yet, oldest first.
        NOT a stream synchronisation: with the polled status mirror the host learns an iteration's status from the
        FIRST thread of its last kernel, so that kernel (the Adam update) may still be running when this returns.
        Whatever reads the parameters next through torch is ordered behind it on the stream; a caller that hands
        the pointers to something else synchronises the stream itself."""
        if self._lag_pending is not None:
            prev, self._lag_pending = self._lag_pending, None
            self._lag_collect(prev, redo_current=False)
        self.flushed, self._lag_ready = self._lag_ready, []
        return self.flushed[-1] if self.flushed else None

    def _ensure_dp(self, group):
        """First sharded step: lay the gradient bucket out for the reduce-scatter, move the four parameter tensors
        into ONE flat buffer (they stay torch Parameters: their storage becomes a view of it) and keep only this
        rank's 1/G of the Adam moments."""
        if self.dp_mode not in ("rs_ag", "allreduce", "sparse"):
            raise ValueError(f"dp_mode must be 'rs_ag', 'allreduce' or 'sparse', not {self.dp_mode!r}")
        G, rank, N = dist.get_world_size(group), dist.get_rank(group), self.N
        if self._dp is not None:
            if self._dp["G"] != G or self._dp["rank"] != rank:
                raise RuntimeError("the process group changed under an engine whose optimiser state is sharded "
                                   f"({self._dp['G']} ranks -> {G}): build a new engine (or remap(reset_state=True))")
            return
        if self._dp_agreed != (G, rank):
            # every rank must run the SAME collective sequence: agree on the scheme once instead of trusting that
            # SLS_DP_MODE / N agree everywhere — MIN and MAX of a mode code (sparse 2, rs_ag 1, allreduce 0; a rank
            # that cannot shard asks for allreduce): sparse only if EVERY rank asks for it, a mix of sparse and a
            # dense scheme is an error on every rank (different collectives would hang), rs_ag needs all ranks able
            # (the sparse scheme's fused Adam and the reduce-scatter layout both need an even N: an odd model falls back
            #  to the all-reduce on every rank alike — N is the same everywhere)
            want = (2 if N % 2 == 0 else 0) if self.dp_mode == "sparse" else (1 if (self.dp_mode == "rs_ag" and N % 2 == 0 and 10 * N < 2 ** 32) else 0)
            t = torch.tensor([want, -want], dtype=torch.int32, device=self.dev)
            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
            lo, hi = int(t[0].item()), -int(t[1].item())
            if hi == 2 and lo != 2:
                raise RuntimeError("keyframe-parallel ranks disagree on the gradient exchange: some ask for dp_mode "
                                   "'sparse', others for a dense scheme (check SLS_DP_MODE on every rank)")
            self._dp_use_rs = lo == 1
            self._dp_agreed = (G, rank)
            self._dp_scheme = lo
        if self._dp_scheme == 2:
            if self._sx is not None and (self._sx["G"], self._sx["rank"]) != (G, rank):
                raise RuntimeError("the process group changed under an engine set up for the sparse exchange "
                                   f"({self._sx['G']} ranks -> {G}): build a new engine (or remap())")
            if self._sx is None:
                lib = _abi.lib()
                nw = int(lib.sls_grad_bitmap_words(N))
                self._sx = {"bitmap": torch.zeros((nw,), dtype=torch.int64, device=self.dev),       # the union (after the OR)
                            "mine": torch.zeros((nw,), dtype=torch.int64, device=self.dev),         # this rank's bitmap
                            "all": torch.zeros((G * nw,), dtype=torch.int64, device=self.dev),      # every rank's
                            "prefix": torch.zeros((nw,), dtype=torch.int32, device=self.dev),
                            "compact": torch.zeros((10 * N,), dtype=torch.float32, device=self.dev),
                            "index": torch.zeros((N,), dtype=torch.int32, device=self.dev),     # the surfel of every slot
                            "send": N,          # slots handed to the SUM collective: all of them until the union's size is known
                            "G": G, "rank": rank}
            return
        if not self._dp_use_rs:
            return
        C = dp_chunk(N, G)
        flat = torch.zeros((G * C,), dtype=torch.float32, device=self.dev)
        m = self.model
        for p, off, w in ((m._xyz, 0, 3), (m._opacity, 3 * N, 1), (m._scaling, 4 * N, 2), (m._rotation, 6 * N, 4)):
            view = flat[off:off + w * N].view(N, w)
            view.copy_(p.data)
            p.data = view
        lo, hi = min(rank * C, 10 * N), min((rank + 1) * C, 10 * N)
        ea, es = torch.zeros((C,), dtype=torch.float32, device=self.dev), torch.zeros((C,), dtype=torch.float32, device=self.dev)
        ea[:hi - lo].copy_(self.exp_avg[lo:hi])
        es[:hi - lo].copy_(self.exp_avg_sq[lo:hi])
        self.exp_avg, self.exp_avg_sq = ea, es                # sharded optimiser state
        self.grads = torch.zeros((G * (C + 4),), dtype=torch.float32, device=self.dev)
        self._dp = {"G": G, "rank": rank, "C": C, "flat": flat, "lo": lo, "hi": hi,
                    "gshard": torch.zeros((C + 4,), dtype=torch.float32, device=self.dev)}

    def _phase_for_exchange(self):
        """1 = the native step stops behind the tile backward (sparse scheme: the union of the touched sets is agreed on
        before the projection's backward runs, which then writes the rows where the collective reads them)"""
        return 1 if self._sx is not None else 0

    def _exchange_and_adam(self, group, status, mirror):
        ev = None
        if self.comm_events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        if self._sx is not None:
            # touched set only: OR of the early bitmaps -> the projection's backward writes the union's rows into their
            # slots and updates everything else -> SUM of the first `send` slots -> Adam on the union
            lib, sx, N = _abi.lib(), self._sx, self.N
            st = torch.cuda.current_stream(self.dev).cuda_stream
            # (RCCL offers no bitwise-OR reduction: the bitmaps are gathered, the library ORs them)
            dist.all_gather_into_tensor(sx["all"], sx["mine"], group=group)
            G = int(sx["all"].numel() // sx["mine"].numel())
            send = int(sx["send"])
            _abi.check(lib.sls_grad_union(N, sx["all"].data_ptr(), G, sx["bitmap"].data_ptr(), send, sx["prefix"].data_ptr(),
                                          status.data_ptr(), st), "sls_grad_union")
            args, cfg = self._last_call
            cfg.phase, cfg.workspace_ready, cfg.apply_adam, cfg.keep_grads = 2, 1, 1, 0
            cfg.union_bitmap, cfg.union_prefix = sx["bitmap"].data_ptr(), sx["prefix"].data_ptr()
            cfg.grad_compact, cfg.grad_compact_index, cfg.grad_compact_capacity = sx["compact"].data_ptr(), sx["index"].data_ptr(), send
            _abi.check(lib.sls_mapping_step(*args), "sls_mapping_step (phase 2)")
            dist.all_reduce(sx["compact"][:10 * send], op=dist.ReduceOp.SUM, group=group)
            if ev:
                ev[1].record()
            xyz, scaling, rotation, opacity = self._params()
            _abi.check(lib.sls_adam_step_union(N, xyz.data_ptr(), opacity.data_ptr(), scaling.data_ptr(), rotation.data_ptr(),
                                               sx["index"].data_ptr(), sx["compact"].data_ptr(), send, self.exp_avg.data_ptr(),
                                               self.exp_avg_sq.data_ptr(), self.lrs[0], self.lrs[1], self.lrs[2], self.lrs[3],
                                               self.betas[0], self.betas[1], self.eps, self.t + 1, status.data_ptr(), mirror,
                                               st), "sls_adam_step_union")
            if ev:
                ev[2].record(); ev[3].record()
            self.exchanged_bytes = 8 * int(sx["mine"].numel()) + 40 * send
        elif self._dp is None:
            dist.all_reduce(self.grads, op=dist.ReduceOp.SUM, group=group)
            if ev:
                ev[1].record()
            self._adam_reduced(status, mirror)
            if ev:
                ev[2].record(); ev[3].record()
            self.exchanged_bytes = 4 * int(self.grads.numel())
        else:
            d = self._dp
            dist.reduce_scatter_tensor(d["gshard"], self.grads, op=dist.ReduceOp.SUM, group=group)
            if ev:
                ev[1].record()
            self._adam_shard(status, mirror)
            if ev:
                ev[2].record()
            C, r = d["C"], d["rank"]
            mine = d["flat"][r * C:(r + 1) * C]
            if d.get("ag_in_place", True):
                try:            # in place: the rank's shard already sits where the collective puts it
                    dist.all_gather_into_tensor(d["flat"], mine, group=group)
                except (RuntimeError, ValueError):     # a backend that refuses aliasing input / output
                    d["ag_in_place"] = False
            if not d.get("ag_in_place", True):
                dist.all_gather_into_tensor(d["flat"], mine.clone(), group=group)
            if ev:
                ev[3].record()
            self.exchanged_bytes = 4 * int(self.grads.numel()) + 4 * C        # reduce-scatter input + the gathered shard
        if ev:
            self.comm_events.append(ev)

    def _adam_groups(self, pieces, params, grad0, lo, flags, status, mirror):
        """sls_adam_step_reduced on the dp_pieces `pieces` of the flat range that starts at element `lo`: `params` = each
        piece's parameter address, `grad0` = the address of element lo's gradient; the moments are this engine's, element
        lo first; `flags` = the address of the two reduced void flags."""
        arr = (_abi.SlsAdamGroup * 4)()
        for k, ((a, b, lr), param) in enumerate(zip(pieces, params)):
            off = 4 * (a - lo)
            arr[k].param, arr[k].grad = param, grad0 + off
            arr[k].exp_avg, arr[k].exp_avg_sq = self.exp_avg.data_ptr() + off, self.exp_avg_sq.data_ptr() + off
            arr[k].numel, arr[k].lr = b - a, lr
        k = len(pieces)
        if k == 0:       # (a rank whose chunk lies beyond 10 N: nothing to update, but it publishes the verdict)
            arr[0].param = arr[0].grad = arr[0].exp_avg = arr[0].exp_avg_sq = grad0
            arr[0].numel, arr[0].lr, k = 0, 0.0, 1
        _abi.check(_abi.lib().sls_adam_step_reduced(arr, k, self.betas[0], self.betas[1], self.eps, self.t + 1, flags,
                                                    status.data_ptr(), mirror,
                                                    torch.cuda.current_stream(self.dev).cuda_stream),
                   "sls_adam_step_reduced")

    def _adam_shard(self, status, mirror):
        """Adam on the flat elements [lo, hi) this rank owns: up to four pieces, one per parameter group the range
        crosses (each has its own learning rate); gradients = the reduce-scattered chunk, moments = the local shard."""
        d = self._dp
        pieces = dp_pieces(self.N, d["lo"], d["hi"], self.lrs)
        self._adam_groups(pieces, [d["flat"].data_ptr() + 4 * a for a, _, _ in pieces], d["gshard"].data_ptr(), d["lo"],
                          d["gshard"].data_ptr() + 4 * d["C"], status, mirror)

    def _adam_reduced(self, status, mirror):
        """Adam on the whole model from the all-reduced flat bucket: the four parameter groups, each in its own tensor."""
        xyz, scaling, rotation, opacity = self._params()
        self._adam_groups(dp_pieces(self.N, 0, 10 * self.N, self.lrs),
                          [p.data_ptr() for p in (xyz, opacity, scaling, rotation)], self.grads.data_ptr(), 0,
                          self.grads.data_ptr() + 4 * 10 * self.N, status, mirror)

    @torch.no_grad()
    def remap(self, keep=None, appended: int = 0, reset_state: bool = True):
        """The model's surfel set changed — call this AFTER replacing the model's parameter tensors, as
        Mapper.densify / the opacity pruning do through cat_tensors_to_optimizer / _prune_optimizer
        (scene/gaussian_model.py:223-316).  `keep`: bool (N_old,), the survivors in their old order (None: all);
        `appended`: number of new surfels that follow them.

        `reset_state=True` (default) is what the reference DOES: `_prune_optimizer` re-files the pruned parameter
        under `optimizer.state[group["name"]]` (scene/gaussian_model.py:237-256), so torch.optim.Adam finds no
        state for the new tensor, and since `update_model` runs densify -> optimize -> prune on every keyframe
        (slam/mapper.py:33-42), each keyframe's `optimize()` starts Adam at step 0 with zero moments.
        `reset_state=False` is what that code evidently intends (and what `cat_tensors_to_optimizer` does when it
        finds a state): the survivors keep their moments, new surfels start from zero, the step count goes on."""
        if self._lag_pending is not None or self._lag_ready:
            self.flush()
        n_old = self.N
        if keep is None:
            keep = torch.ones((n_old,), dtype=torch.bool, device=self.dev)
        keep = keep.to(self.dev).reshape(-1)
        if keep.dtype != torch.bool or keep.numel() != n_old or appended < 0:
            raise ValueError("keep must be a bool mask over the engine's current surfels, appended >= 0")
        n_keep = int(keep.sum().item())
        n_new = n_keep + int(appended)
        if int(self.model._xyz.shape[0]) != n_new:
            raise RuntimeError(f"the model holds {int(self.model._xyz.shape[0])} surfels, keep/appended describe {n_new}")
        if self._dp is not None and not reset_state:      # (before any state is touched: the engine stays consistent)
            raise RuntimeError("remap(reset_state=False) is not available once the optimiser state is sharded "
                               "(keyframe-parallel mode rs_ag): use reset_state=True or dp_mode='allreduce'")

        if reset_state:
            self.exp_avg = torch.zeros((10 * n_new,), dtype=torch.float32, device=self.dev)
            self.exp_avg_sq = torch.zeros((10 * n_new,), dtype=torch.float32, device=self.dev)
            self.t = 0
        else:
            self.exp_avg = carry_bucket(self.exp_avg, keep, n_new)
            self.exp_avg_sq = carry_bucket(self.exp_avg_sq, keep, n_new)
        self._dp_agreed = None
        self._sx = None
        self._dp = None                               # re-sharded at the next keyframe-parallel step
        self.N = n_new
        self._set_order_ages()
        self.grads = torch.zeros((10 * n_new + 2,), dtype=torch.float32, device=self.dev)
        self.workspace = None                        # sized by N: rebuilt at the next step
        self._orders.clear()                         # surfel indices changed: every depth order and predicted scale is void
        self._det_two_pass_next = True
        self._pose_scratch = None                    # (sized by N)
        self._params()

    @torch.no_grad()
    def resize(self, n_new: int) -> None:
        """The surfel set changed size and the caller brings the optimiser state itself (fused_mapper.fused_optimize reads
        it from optimizer.state before every run, as the reference's densify / prune helpers leave it): everything that
        does not depend on N stays — the pinned status mirrors, the events, the keyframes' launch orders of the tile
        backward — and what does is re-used while it is large enough (buckets, workspace and depth-order buffers are
        allocated with a quarter of head room: a local model grows by < 1 % per keyframe).  Depth orders are void
        (surfel indices moved); moments and step count are whatever the caller writes next.  Single-GPU path only."""
        if self._lag_pending is not None or self._lag_ready:
            self.flush()
        if self._dp is not None or self._sx is not None:
            raise RuntimeError("resize() is for the single-GPU engine; keyframe-parallel state is laid out by N: use remap()")
        n_new = int(n_new)
        if int(self.model._xyz.shape[0]) != n_new:
            raise RuntimeError(f"the model holds {int(self.model._xyz.shape[0])} surfels, not {n_new}")
        n10 = 10 * n_new
        store = self._bucket_store
        if store is None or store[0].numel() < n10 + 2:
            room = n10 + n10 // 4 + 2
            store = [torch.zeros((room,), dtype=torch.float32, device=self.dev) for _ in range(3)]
            self._bucket_store = store
        self.grads, self.exp_avg, self.exp_avg_sq = store[0][:n10 + 2], store[1][:n10], store[2][:n10]
        self.grads.zero_()
        self.N, self.t = n_new, 0
        self._set_order_ages()
        for ent in self._orders.values():
            ent.stamp = ent.det_prev = None                 # the order itself: from scratch at the keyframe's next visit
            if ent.order.numel() < n_new:
                ent.order = torch.empty((n_new + n_new // 4,), dtype=torch.int32, device=self.dev)
        self._det_two_pass_next = True
        self._ws_ready = False                              # (the records' region moved with N: zeroed at the next step)
        self._params()

    def allmap(self, H, W) -> torch.Tensor:
        """Copy of the last iteration's allmap (7,H,W) out of the workspace.  With depth_ratio == 0 the mapper's
        loss neither reads nor differentiates the median / distortion planes (gaussian_renderer/__init__.py:79-86),
        and the native iteration does not track them: planes 5 and 6 are zeros then (render() through
        GaussianRasterizer always fills all seven)."""
        off = int(self.allmap_ptr.value) - self.workspace.data_ptr()
        return self.workspace[off:off + 7 * H * W * 4].view(torch.float32).view(7, H, W).clone()
