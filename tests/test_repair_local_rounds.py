"""The depth-order repair with further rounds only where a window needs them (sls_sort.hip, resort_merge_kernel ESC).

CPU part: the NumPy model of the scheme (tests/repair_ref.py) against k global rounds — the k launches it replaces —
and against np.argsort(kind="stable"), on nearly sorted orders.  What one element can travel (in positions, the old
order cut into aligned windows of 1024):
    * k rounds are 2k - 1 levels of merges; an element sitting at offset o of its aligned window that has to move
      FORWARD reaches the end of its window in the window sort and 512 positions more with every level:
      1023 - o + 512 (2k - 1) positions.  So k rounds always reach 512 (2k - 1) >= 512 k, and never 1024 k + 512.
      Backward the same, mirrored.
    * Hence the classes below: up to 512, 513..1023, 1025..1535 are placed where the number of rounds that reach them is
      known; "beyond" is 1024 k + 512 and more, where k rounds MUST report failure.  Between 512 (2k - 1) and
      1024 k + 512 the outcome depends on where the element sits; there, as everywhere, the one-launch form must give
      what the k launches give, verdict included.
GPU part: through MappingEngine, as tests/test_gpu_parity.py::test_depth_order_repair_rounds does."""
import numpy as np
import pytest

import repair_ref as ref

SIZES = (1000, 1024, 2049, 6181, 7168)
ROUNDS = (1, 2, 3, 4)


def _scene(N, seed):
    """keys_by_surfel (with ties: the surfel index breaks them) and the exact order"""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.integers(0, 1 << 24, size=N).astype(np.uint32) >> 3)      # (ties among neighbours)
    surfel_of_rank = rng.permutation(N)
    keys_by_surfel = np.empty(N, dtype=np.uint32)
    keys_by_surfel[surfel_of_rank] = keys
    exact = np.argsort(keys_by_surfel, kind="stable")
    return keys_by_surfel, exact


def _move(order, src, dst):
    """the element at position src of `order` sits at position dst instead: it has |src - dst| positions to travel"""
    o = list(order)
    g = o.pop(src)
    o.insert(dst, g)
    return np.asarray(o)


def _jitter(order, rng, reach=40):
    """every element a little out of place, as between two iterations on a keyframe"""
    rank = np.arange(order.size) + rng.uniform(-reach, reach, order.size)
    return order[np.argsort(rank, kind="stable")]


def _check(keys_by_surfel, exact, old, k, must=None):
    comp = ref.window_sort(keys_by_surfel, old)
    g_out, g_ok = ref.global_rounds(comp, k)
    l_out, l_ok, esc, merges = ref.local_rounds(comp, k)
    assert np.array_equal(l_out, g_out), "not what k launches leave"
    assert l_ok == g_ok
    if l_ok:
        assert np.array_equal((l_out & np.uint64(0xFFFFFFFF)).astype(np.int64), exact)
    else:
        assert not np.array_equal((l_out & np.uint64(0xFFFFFFFF)).astype(np.int64), exact)
    if must is not None:
        assert l_ok == must, (k, must)
    if k == 1:
        assert esc == 0
    assert merges <= esc * k * (2 * k - 1)          # (all the levels of a cone: 2k - 1 + 2k - 2 + ... + 1 merges)
    return l_ok, esc


def _placements(N):
    """(name, first position, last position) of the window the displaced elements sit in (in the OLD order)"""
    nA = (N + ref.W - 1) // ref.W
    out = [("first", 0, min(ref.W, N) - 1), ("last", (nA - 1) * ref.W, N - 1)]
    if nA >= 3:
        mid = nA // 2
        out.append(("middle", mid * ref.W, (mid + 1) * ref.W - 1))
    return out


@pytest.mark.parametrize("k", ROUNDS)
@pytest.mark.parametrize("N", SIZES)
def test_model_matches_global_rounds_by_displacement_class(N, k):
    keys_by_surfel, exact = _scene(N, N + k)
    rng = np.random.default_rng(7 * N + k)
    ran = 0
    for _, a0, a1 in _placements(N):
        for forward in (True, False):
            # the element sits at the end of its window if it has to move forward (the window sort does not help it),
            # at the start if backward
            src = a1 if forward else a0
            room = (N - 1 - src) if forward else src
            for lo, hi in ((1, 512), (513, 1023), (1025, 1535), (1024 * k + 512, 1024 * k + 900)):
                hi = min(hi, room)
                if hi < lo:
                    continue          # (the order is too short for an element to travel that far from here)
                for D in {lo, hi, int(rng.integers(lo, hi + 1))}:
                    dst = src + D if forward else src - D
                    old = _move(exact, dst, src)          # the element of rank dst sits at src
                    # the far end of its aligned window: the window sort does not move it, the levels 512 positions each
                    must = D <= 512 * (2 * k - 1)
                    _check(keys_by_surfel, exact, old, k, must)
                    # the same under the jitter of a real step, and with three travellers from the same window
                    old2 = _jitter(old, rng)
                    _check(keys_by_surfel, exact, old2, k)
                    old3 = old
                    for extra in (3, 11):
                        s2 = min(max(src - extra if forward else src + extra, a0), a1)
                        d2 = min(max(s2 + D // 2 if forward else s2 - D // 2, 0), N - 1)
                        old3 = _move(old3, d2, s2)
                    _check(keys_by_surfel, exact, old3, k)
                    ran += 1
    if N <= ref.W:          # one window: the window sort alone brings any old order home
        assert ran == 0
        _check(keys_by_surfel, exact, rng.permutation(N), k, True)
    else:
        assert ran > 0


@pytest.mark.parametrize("k", ROUNDS)
def test_model_beyond_reach_reports_failure(k):
    """an element 1024 k + 512 positions and more from its place: k rounds cannot bring it there wherever it sits"""
    N = 7168
    keys_by_surfel, exact = _scene(N, 99 + k)
    rng = np.random.default_rng(k)
    D = 1024 * k + 512
    for _ in range(6):
        src = int(rng.integers(0, N - D))
        for old in (_move(exact, src + D, src), _move(exact, src, src + D)):
            ok, _ = _check(keys_by_surfel, exact, old, k, must=False)
            assert not ok


@pytest.mark.parametrize("k", ROUNDS)
@pytest.mark.parametrize("N", SIZES)
def test_model_matches_global_rounds_on_noisy_orders(N, k):
    """nearly sorted by noise of growing reach: verdict and order of the one-launch form are those of k launches; a quiet
    order escalates nowhere, and an escalation stays near the boundaries that are out of order"""
    keys_by_surfel, exact = _scene(N, 1000 + N + k)
    rng = np.random.default_rng(N * 31 + k)
    for reach in (0, 100, 400, 700, 1500, 4000):
        old = _jitter(exact, rng, reach) if reach else exact
        ok, esc = _check(keys_by_surfel, exact, old, k)
        if reach <= 100:
            assert ok and esc == 0          # (a step's usual motion: the cost of one round)
    # one disturbance in the middle of a long order: at most the windows whose cone holds the boundary escalate
    if N >= 6181 and k >= 2:
        old = _move(exact, 3 * ref.W + 900 + 700, 3 * ref.W + 900)
        ok, esc = _check(keys_by_surfel, exact, old, k, must=True)
        assert 1 <= esc <= 2 * (2 * k - 2)


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _engines(device, sc, rounds_list):
    from splat_loam_amd.engine import MappingEngine
    from splat_loam_amd.mapping import MappingConfig
    from splat_loam_amd.scene import SurfelModel
    out = []
    for rounds in rounds_list:
        m = SurfelModel.from_activated(sc["means"], sc["scales"], sc["rots"], sc["opac"], device=str(device))
        e = MappingEngine(m, MappingConfig())
        e.reuse_depth_order = rounds > 0
        e.deterministic = True          # (bit-identical trajectories: the orders can be compared at all)
        e._repair_rounds, e._repair_until = max(rounds, 1), 10 ** 9
        out.append((e, m))
    return out


@pytest.fixture(scope="module", params=[6181, 30000])
def repair_scene(request, device):
    """the scene, its camera and the from-scratch engine's state after two steps (shared, never modified)"""
    import torch
    from splat_loam_amd import synth
    from splat_loam_amd.scene import Camera
    N, H, W = request.param, 32, 512
    sc = synth.make_scene(N, H, W, seed=16, range_lo=2.0, range_hi=25.0)
    depth, valid = synth.make_targets(H, W, sc)
    cam = Camera(sc["K"], depth, None, valid, None, data_device=str(device))
    (e, m), = _engines(device, sc, (0,))
    e.step(cam), e.step(cam)
    order = e._orders[id(cam)].order.cpu().numpy().astype(np.int64)
    rng_of = torch.linalg.norm(m._xyz.detach(), dim=1).cpu().numpy().astype(np.float64)
    return {"N": N, "sc": sc, "cam": cam, "order": order, "range": rng_of}


# (name, position in the order after two steps, positions to travel, rounds that cannot reach it)
# sources sit 24 positions from the far end of their aligned window: a forward traveller is carried
# 23 + 512 (2k - 1) positions by k rounds, so 800 and 1280 need two rounds, 2000 needs three, 300 one; backward mirrored.
def _cases(N):
    nA = (N + 1023) // 1024
    mid = nA // 2
    return [
        ("middle_fwd_300", mid * 1024 + 1000, 300, ()),
        ("middle_fwd_800", mid * 1024 + 1000, 800, (1,)),
        ("middle_fwd_1280", mid * 1024 + 1000, 1280, (1,)),
        ("first_window_fwd_2000", 1000, 2000, (1, 2)),
        ("into_first_window_bwd_800", 1024 + 24, -800, (1,)),
        ("into_ragged_last_window_fwd_800", (nA - 2) * 1024 + 1000 if N % 1024 > 900 or N % 1024 == 0 else (nA - 3) * 1024 + 1000, 800, (1,)),
        ("out_of_ragged_last_window_bwd_1280", (nA - 1) * 1024 + 24, -1280, (1,)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(7))
def test_engine_repairs_in_one_launch(device, repair_scene, case):
    """Orders, losses and parameters of the engines that repair with k = 1..4 rounds equal the from-scratch engine's bit
    for bit; an engine voids and repeats an iteration exactly where its rounds cannot reach."""
    import torch
    s = repair_scene
    N, cam = s["N"], s["cam"]
    name, src, D, failing = _cases(N)[case]
    dst = src + D
    assert 0 <= src < N and 0 < dst < N - 1, name
    g = int(s["order"][src])
    # the surfel's new range: between the ranges of the two surfels around its new place
    a, b = (dst, dst + 1) if D > 0 else (dst - 1, dst)
    new_range = 0.5 * (s["range"][s["order"][a]] + s["range"][s["order"][b]])
    f = float(new_range / s["range"][g])
    engines = _engines(device, s["sc"], (0, 1, 2, 3, 4))
    losses = []
    for e, m in engines:
        ls = [e.step(cam)["loss"], e.step(cam)["loss"]]
        with torch.no_grad():
            m._xyz[g] *= f
        ls += [e.step(cam)["loss"], e.step(cam)["loss"]]
        losses.append(ls)
    o0 = engines[0][0]._orders[id(cam)].order.cpu().numpy()
    moved = abs(int(np.nonzero(o0 == g)[0][0]) - src)
    print(f"{name} N={N}: surfel {g} travelled {moved} positions; repeated_resort "
          f"{[e.stats['repeated_resort'] for e, _ in engines]}")
    assert abs(moved - abs(D)) <= 100, "the perturbation did not move the surfel as planned"
    p0 = [p.detach().cpu().numpy() for p in (engines[0][1]._xyz, engines[0][1]._scaling, engines[0][1]._rotation, engines[0][1]._opacity)]
    for k, (e, m) in enumerate(engines):
        assert e.stats["repeated_resort"] == (1 if k in failing else 0), (name, k, e.stats)
        assert np.array_equal(e._orders[id(cam)].order.cpu().numpy(), o0), (name, k)
        assert losses[k] == losses[0], (name, k, losses)
        for a_, b_ in zip(p0, (m._xyz, m._scaling, m._rotation, m._opacity)):
            assert np.array_equal(a_, b_.detach().cpu().numpy()), (name, k)
