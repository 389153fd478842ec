"""Keyframe-parallel mapping at G = 8 (BASELINE config 5: one keyframe per rank, gradients summed over the ranks), pinned
to a float64 reference.

Eight gloo ranks share cuda:0.  Each spawn builds several engines one after another in the same process group (the
"legs"), and every rank dumps what it held at every step: the parameters the step started from, the reduced gradient
(its own chunk under rs_ag, the whole bucket under allreduce, the union's rows under sparse) and its Adam moments.  The
parent then checks, step by step:

  1. the reduced gradient against the float64 sum of the eight single-keyframe gradients at the same parameters
     (MappingEngine._enqueue(apply_adam=False), the regulariser on keyframe 0 only, as the two-rank tests do);
  2. the parameters and moments after the step against a float64 Adam fed with the float32 reduced gradient the ranks
     held, chained from the dumped parameters and moments (a free-running reference would let one sign flip of a
     rounding-noise gradient become a whole-lr step).

The two-rank tests cannot see a rank >= 1 that updates its shard with the wrong learning rate, moment offset or step
count: the all-gather copies the error to every replica, and the reduced gradient is unchanged.  At G = 8 and N = 50 000
(C = 62 500) two chunk edges also fall inside xyz rows, which the reduce-scatter layout of preprocess_bwd handles apart.
"""
import datetime
import hashlib
import os
import socket
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G = 8
LRS = (5e-4, 5e-2, 5e-3, 1e-3)
BETAS = (0.9, 0.999)
EPS = 1e-15
STEPS = 3
C5 = dict(N=50000, H=64, W=1024)          # config 5's geometry: 8 keyframes of a 64x1024 LiDAR window


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _scene(N, H, W):
    from splat_loam_amd import synth
    sc = synth.make_scene(N, H, W, seed=31, range_lo=2.0, range_hi=15.0)
    depth, valid = synth.make_targets(H, W, sc)
    return sc, depth, valid


def _camera(scene, k, device):
    from splat_loam_amd import synth
    from splat_loam_amd.scene import Camera
    sc, depth, valid = scene
    return Camera(sc["K"], depth, None, valid, synth.keyframe_poses(G)[k], data_device=device)


def _flat_params(model):
    """The four raw parameter tensors in the flat bucket order [xyz 3N | opacity N | scaling 2N | rotation 4N]."""
    return torch.cat([model._xyz.detach().reshape(-1), model._opacity.detach().reshape(-1),
                      model._scaling.detach().reshape(-1), model._rotation.detach().reshape(-1)]).cpu().numpy()


def _groups(N):
    return ((0, 3 * N, LRS[0]), (3 * N, 4 * N, LRS[1]), (4 * N, 6 * N, LRS[2]), (6 * N, 10 * N, LRS[3]))


def _reduced(eng):
    """The summed gradient as this rank holds it, in the flat bucket layout: its own chunk [lo, hi) (reduce-scatter),
    the whole bucket (all-reduce) or the union's rows scattered back (sparse; + the union as a bool mask over surfels)."""
    N = eng.N
    if eng._sx is not None:
        sx = eng._sx
        bits = np.unpackbits(sx["bitmap"][:-2].cpu().numpy().view(np.uint8), bitorder="little")[:N].astype(bool)
        rows = np.zeros((N, 10), np.float32)
        k = int(bits.sum())
        rows[bits] = sx["compact"][:10 * k].cpu().numpy().reshape(k, 10)
        flat = np.concatenate([rows[:, 0:3].reshape(-1), rows[:, 3], rows[:, 4:6].reshape(-1), rows[:, 6:10].reshape(-1)])
        return flat, 0, 10 * N, bits
    if eng._dp is None:
        return eng.grads[:-2].cpu().numpy(), 0, 10 * N, None
    d = eng._dp
    return d["gshard"][:d["hi"] - d["lo"]].cpu().numpy(), d["lo"], d["hi"], None


def _run_leg(rank, leg):
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import SurfelModel
    N, H, W, steps = leg["N"], leg["H"], leg["W"], leg.get("steps", STEPS)
    scene = _scene(N, H, W)
    cam = _camera(scene, rank, "cuda:0")
    sc = scene[0]
    model = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device="cuda:0")
    eng = MappingEngine(model, MappingConfig())
    eng.dp_mode = leg["scheme"][rank] if isinstance(leg["scheme"], (list, tuple)) else leg["scheme"]
    if leg.get("overflow_rank") == rank:
        eng.capacity = 1024           # this rank's instance buffers overflow: EVERY rank must void and repeat
    out = {}
    t0 = time.perf_counter()
    if leg.get("expect_error"):
        try:
            eng.step(cam)
            out["error"] = np.array("")
        except RuntimeError as e:
            out["error"] = np.array(str(e))
        return out
    if leg.get("lagged"):
        seen = [eng.step(cam, sync="lagged") for _ in range(steps)]
        last = eng.flush()
        handed = seen[1:] + list(eng.flushed)
        out.update(first_none=seen[0] is None, handed=len(handed), handed_void=sum(bool(s["overflow"]) for s in handed),
                   last_clean=last is not None and not last["overflow"])
    else:
        rec = {k: [] for k in ("p", "g", "m", "v", "bits", "d_p", "d_g", "d_m", "d_v", "d_bits", "outside_union",
                               "exchange_count", "send")}
        for s in range(steps):
            if leg.get("shrink_send") and s == 1:
                # the same host-side capacity on every rank (it follows the group's union): half the union's size, so the
                # union no longer fits the SUM collective -> bit 2 voids the iteration everywhere, repeated with more room
                eng._sx["send"] = max(1, int(eng.last["exchange_count"]) // 2)
            p = _flat_params(model)
            st = eng.step(cam)
            g, lo, hi, bits = _reduced(eng)
            m, v = eng.exp_avg[:hi - lo].cpu().numpy(), eng.exp_avg_sq[:hi - lo].cpu().numpy()
            # every rank keeps what only it holds (its chunk); of what every rank holds a copy of, rank 0 keeps the
            # arrays and every rank a digest (replicas must agree to the bit)
            keep = eng._dp is not None or rank == 0
            for k, a in (("p", p), ("g", g), ("m", m), ("v", v), ("bits", bits)):
                if a is None:
                    continue
                rec["d_" + k].append(_digest(a))
                if keep and (k != "p" or rank == 0):
                    rec[k].append(a)
            rec["outside_union"].append(bool(st["outside_union"]))
            rec["exchange_count"].append(int(st["exchange_count"]))
            rec["send"].append(int(eng._sx["send"]) if eng._sx is not None else -1)
            out.update(lo=lo, hi=hi)
        for k, a in rec.items():
            if a:
                out[k] = np.stack(a) if isinstance(a[0], np.ndarray) else np.array(a)
        out["C"] = eng._dp["C"] if eng._dp is not None else -1
    final = _flat_params(model)
    out.update(d_final=_digest(final), t=eng.t, sharded_state=int(eng._dp is not None), sparse_state=int(eng._sx is not None),
               state_len=int(eng.exp_avg.numel()), seconds=time.perf_counter() - t0,
               **{"stat_" + k: v for k, v in eng.stats.items()})
    if rank == 0:
        out["final"] = final
    return out


def _rank_main(rank, port, out_dir, legs):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    # (a rank that raises leaves the others in a collective: they give up after this long instead of gloo's 30 min)
    dist.init_process_group("gloo", rank=rank, world_size=G, timeout=datetime.timedelta(seconds=180))
    try:
        for leg in legs:
            np.savez(os.path.join(out_dir, f"{leg['name']}_r{rank}.npz"), **_run_leg(rank, leg))
    finally:
        dist.destroy_process_group()


def _spawn(tmp_path, legs):
    import torch.multiprocessing as mp
    mp.spawn(_rank_main, args=(_free_port(), str(tmp_path), legs), nprocs=G, join=True)
    return {leg["name"]: [np.load(tmp_path / f"{leg['name']}_r{r}.npz") for r in range(G)] for leg in legs}


def _check_replicas(name, R, steps=STEPS):
    """Every rank ends with the same parameters and step count — and started every step from the same ones."""
    assert all(int(r["t"]) == steps for r in R), f"{name}: step counts {[int(r['t']) for r in R]}"
    assert len({str(r["d_final"]) for r in R}) == 1, f"{name}: replicas diverged"
    if "d_p" in R[0].files:
        for s in range(steps):
            assert len({str(r["d_p"][s]) for r in R}) == 1, f"{name}: replicas diverged before step {s}"


def _keyframe_sum(N, H, W, flat, device):
    """float64 sum over the eight keyframes of the single-keyframe gradient at the flat parameters `flat`."""
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import SurfelModel
    scene = _scene(N, H, W)
    total = np.zeros(10 * N, np.float64)
    for k in range(G):
        cam = _camera(scene, k, str(device))
        model = SurfelModel(flat[:3 * N].reshape(N, 3), flat[4 * N:6 * N].reshape(N, 2), flat[6 * N:].reshape(N, 4),
                            flat[3 * N:4 * N].reshape(N, 1), device=str(device))
        eng = MappingEngine(model, MappingConfig())
        eng._enqueue(cam, apply_adam=False, with_regulariser=(k == 0))
        flags = int(eng.status[1].item())
        if flags & 1:       # instance buffers too small: the engine's own protocol, with the room it asked for
            eng.capacity = eng._grown(int(eng.status[0].item()) & 0xFFFFFFFF)
            eng.workspace = None
            eng._enqueue(cam, apply_adam=False, with_regulariser=(k == 0), allow_reuse=False)
            flags = int(eng.status[1].item())
        assert flags == 0, f"reference keyframe {k}: void iteration ({flags})"
        total += eng.grads[:-2].cpu().numpy().astype(np.float64)
    return total


def _check_against_float64(name, R, leg, device):
    """Per step: reduced gradient vs the float64 keyframe sum, then parameters and moments vs a float64 Adam step on
    that float32 gradient.  Returns the number of elements compared in each check."""
    N, H, W, steps = leg["N"], leg["H"], leg["W"], leg.get("steps", STEPS)
    sharded = int(R[0]["sharded_state"]) == 1
    sparse = int(R[0]["sparse_state"]) == 1
    P = np.concatenate([R[0]["p"], R[0]["final"][None]]).astype(np.float64)
    lr = np.concatenate([np.full(b - a, g) for a, b, g in _groups(N)])
    b1, b2 = BETAS
    counts = {"grad": 0, "superset": 0, "superset_nonzero": 0, "param": 0, "moment": 0}
    m_prev = v_prev = np.zeros(10 * N, np.float64)
    for s in range(steps):
        if sharded:
            # the eight chunks in rank order: lo = r*C (clamped to 10N for a rank whose chunk lies beyond the model)
            from splat_loam_amd.engine import dp_chunk
            C = dp_chunk(N, G)
            for r in range(G):
                assert int(R[r]["C"]) == C
                assert (int(R[r]["lo"]), int(R[r]["hi"])) == (min(r * C, 10 * N), min((r + 1) * C, 10 * N)), f"{name}: rank {r}"
                assert int(R[r]["state_len"]) == C, f"{name}: rank {r} keeps more than its shard of the moments"
            assert int(R[G - 1]["hi"]) == 10 * N
            red, m, v = (np.concatenate([R[r][k][s] for r in range(G)]).astype(np.float64) for k in ("g", "m", "v"))
        else:
            for k in ("g", "m", "v"):
                assert len({str(r["d_" + k][s]) for r in R}) == 1, f"{name}: ranks hold different {k} at step {s}"
            red, m, v = (R[0][k][s].astype(np.float64) for k in ("g", "m", "v"))
        assert red.shape == (10 * N,) and m.shape == (10 * N,)
        total = _keyframe_sum(N, H, W, R[0]["p"][s], device)
        scale = np.abs(total).max()
        err = np.abs(red - total).max()
        assert err <= 1e-5 * scale, f"{name} step {s}: reduced gradient off by {err} (scale {scale})"
        counts["grad"] += red.size
        if sparse:
            assert len({str(r["d_bits"][s]) for r in R}) == 1, f"{name}: ranks agreed on different unions at step {s}"
            assert not any(bool(r["outside_union"][s]) for r in R), f"{name}: bit 5 rose at step {s}"
            bits = R[0]["bits"][s]
            assert int(bits.sum()) == int(R[0]["exchange_count"][s])
            in_union = np.concatenate([np.repeat(bits, 3), bits, np.repeat(bits, 2), np.repeat(bits, 4)])
            stray = (total != 0) & ~in_union
            assert not stray.any(), f"{name} step {s}: {int(stray.sum())} non-zero gradient elements outside the union"
            counts["superset"] += total.size
            counts["superset_nonzero"] += int((total != 0).sum())
        # float64 Adam on the float32 reduced gradient, from the dumped parameters and moments of the step before
        t = s + 1
        m_ref = b1 * m_prev + (1 - b1) * red
        v_ref = b2 * v_prev + (1 - b2) * red * red
        p_ref = P[s] - lr / (1 - b1 ** t) * m_ref / (np.sqrt(v_ref) / np.sqrt(1 - b2 ** t) + EPS)
        ulp = np.spacing(np.abs(p_ref).astype(np.float32)).astype(np.float64)
        tol = 2 * ulp + 1e-5 * np.abs(p_ref - P[s])
        bad = np.abs(P[s + 1] - p_ref) > tol
        if bad.any():
            i = int(np.argmax(np.abs(P[s + 1] - p_ref) - tol))
            pytest.fail(f"{name} step {s}: {int(bad.sum())} parameters off the float64 Adam step, e.g. element {i}: "
                        f"{P[s + 1][i]!r} vs {p_ref[i]!r} (from {P[s][i]!r}, gradient {red[i]!r})")
        counts["param"] += p_ref.size
        for a, b, _ in _groups(N):
            for got, ref, what in ((m, m_ref, "exp_avg"), (v, v_ref, "exp_avg_sq")):
                e, sc = np.abs(got[a:b] - ref[a:b]).max(), np.abs(ref[a:b]).max()
                assert e <= 2e-6 * sc, f"{name} step {s}: {what}[{a}:{b}] off by {e} (scale {sc})"
                counts["moment"] += b - a
        m_prev, v_prev = m, v
    return counts


# every leg the reference checks, in one spawn: float atomics (the default accumulation)
LEGS_REFERENCE = [
    dict(name="c5_rs_ag", scheme="rs_ag", **C5),
    dict(name="c5_allreduce", scheme="allreduce", **C5),
    dict(name="c5_sparse", scheme="sparse", **C5),
    dict(name="padded", scheme="rs_ag", N=50002, H=64, W=1024),     # G*C = 500 032 > 10N: the last chunk is padded
    dict(name="tiny2", scheme="rs_ag", N=2, H=16, W=64),            # C = 4: ranks 5-7 own nothing (k == 0)
    dict(name="tiny8", scheme="rs_ag", N=8, H=16, W=64),            # C = 12: chunk edges at 3N and 6N; rank 7 owns nothing
    dict(name="odd_rs_ag", scheme="rs_ag", N=4999, H=32, W=256),    # odd N: every rank falls back to the all-reduce
    dict(name="odd_sparse", scheme="sparse", N=4999, H=32, W=256),
]
LEG_DISAGREE = dict(name="disagree", scheme=["rs_ag"] * 3 + ["sparse"] + ["rs_ag"] * 4, N=64, H=16, W=64,
                    expect_error=True)


@pytest.mark.timeout(600)
def test_eight_ranks_match_a_float64_reference(device, tmp_path):
    """Config 5 as far as one GPU allows: 8 ranks, 50 000 surfels, 64x1024, three steps of each exchange scheme, plus the
    awkward chunk layouts (padded last chunk, empty chunks, chunk edges on group edges, the odd-N fall-back) — every
    step's reduced gradient, parameters and moments against float64.  Last, ranks that disagree on the scheme (one asks
    for sparse, seven for rs_ag) must all raise instead of entering different collectives."""
    from splat_loam_amd.engine import dp_chunk
    # the layouts the legs are meant to reach
    C = dp_chunk(C5["N"], G)
    assert C == 62500 and sum(1 for r in range(1, G) if r * C < 3 * C5["N"] and r * C % 3) == 2
    assert G * dp_chunk(50002, G) > 10 * 50002
    assert dp_chunk(2, G) == 4 and [r for r in range(G) if r * 4 >= 20] == [5, 6, 7]
    assert dp_chunk(8, G) == 12 and {24, 48} <= {r * 12 for r in range(G)}
    t0 = time.perf_counter()
    out = _spawn(tmp_path, LEGS_REFERENCE + [LEG_DISAGREE])
    spawn_s = time.perf_counter() - t0
    for leg in LEGS_REFERENCE:
        name, R = leg["name"], out[leg["name"]]
        _check_replicas(name, R)
        want_rs = leg["scheme"] == "rs_ag" and leg["N"] % 2 == 0
        want_sparse = leg["scheme"] == "sparse" and leg["N"] % 2 == 0
        for r in R:
            assert int(r["sharded_state"]) == int(want_rs) and int(r["sparse_state"]) == int(want_sparse), name
        t1 = time.perf_counter()
        counts = _check_against_float64(name, R, leg, device)
        print(f"\n[G=8] {name}: N={leg['N']} {leg['H']}x{leg['W']}, {max(float(r['seconds']) for r in R):.2f} s on the "
              f"ranks, reference {time.perf_counter() - t1:.2f} s; elements compared over {STEPS} steps: {counts}"
              + (f"; union rows per step {[int(x) for x in R[0]['exchange_count']]}" if want_sparse else ""))
    errors = [str(r["error"]) for r in out["disagree"]]
    assert all("disagree" in e for e in errors), f"not every rank refused the mixed schemes: {errors}"
    print(f"[G=8] spawn of {len(LEGS_REFERENCE) + 1} legs: {spawn_s:.1f} s")


@pytest.mark.timeout(600)
def test_eight_ranks_void_and_repeat_together(device, tmp_path, monkeypatch):
    """Integer-atomic accumulation (SLS_DETERMINISTIC=1) makes every run of a scheme feed the collectives the same
    inputs, so a run in which one middle rank (5) overflows its instance buffers — all eight void the iteration and
    repeat it — ends on the clean run's parameters to the bit, synchronous and lagged; so does a sparse run whose
    collective is cut to half the union (bit 2: "union too small", repeated with more room).  The clean runs are held
    to the float64 reference as well.  (No equality ACROSS schemes: with eight ranks gloo may add an element's terms in
    an order that depends on where it lies in the buffer.)"""
    monkeypatch.setenv("SLS_DETERMINISTIC", "1")
    legs = []
    for scheme in ("rs_ag", "allreduce", "sparse"):
        legs += [dict(name=f"clean_{scheme}", scheme=scheme, **C5),
                 dict(name=f"overflow_{scheme}", scheme=scheme, overflow_rank=5, **C5)]
    legs += [dict(name="lagged_rs_ag", scheme="rs_ag", overflow_rank=5, lagged=True, **C5),
             dict(name="shrunk_sparse", scheme="sparse", shrink_send=True, **C5)]
    t0 = time.perf_counter()
    out = _spawn(tmp_path, legs)
    spawn_s = time.perf_counter() - t0
    for leg in legs:
        _check_replicas(leg["name"], out[leg["name"]])
    for scheme in ("rs_ag", "allreduce", "sparse"):
        clean, over = out[f"clean_{scheme}"], out[f"overflow_{scheme}"]
        assert all(int(r["stat_repeated_too_small"]) == 0 for r in clean), f"clean_{scheme} voided an iteration"
        assert all(int(r["stat_repeated_too_small"]) >= 1 for r in over), f"overflow_{scheme}: not every rank repeated"
        assert np.array_equal(over[0]["final"], clean[0]["final"]), f"{scheme}: the repeated iteration changed the parameters"
        counts = _check_against_float64(f"clean_{scheme}", clean, dict(scheme=scheme, **C5), device)
        print(f"\n[G=8, deterministic] clean_{scheme}: elements compared over {STEPS} steps: {counts}")
    lag = out["lagged_rs_ag"]
    for r in lag:
        assert bool(r["first_none"]) and bool(r["last_clean"]), "lagged: flush() did not end on a clean iteration"
        assert int(r["handed"]) == STEPS and int(r["handed_void"]) == 0
        assert int(r["stat_repeated_too_small"]) >= 1, "lagged: not every rank repeated"
    assert np.array_equal(lag[0]["final"], out["clean_rs_ag"][0]["final"]), "lagged: the parameters differ from the clean run"
    shrunk = out["shrunk_sparse"]
    assert all(int(r["stat_repeated_exchange"]) >= 1 for r in shrunk), "shrunk_sparse: the union fitted the halved collective"
    assert all(int(r["send"][1]) >= int(r["exchange_count"][1]) for r in shrunk)
    assert np.array_equal(shrunk[0]["final"], out["clean_sparse"][0]["final"]), "shrunk_sparse: the repeat changed the parameters"
    print(f"[G=8, deterministic] spawn of {len(legs)} legs: {spawn_s:.1f} s; union rows per step "
          f"{[int(x) for x in out['clean_sparse'][0]['exchange_count']]}")
