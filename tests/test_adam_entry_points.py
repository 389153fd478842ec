"""Every way into the library's one Adam update rule (adam_one, sls_common.hpp) through the C ABI, element by element:
sls_adam_step, _guarded and _reduced (adam_kernel), sls_adam_step_sparse and _union (sls_exchange.hip) and FusedAdam's
split into launches — against the float64 reference and the derived float32 bounds of tests/adam_ref.py, chained one step at
a time from the float32 state the device produced; entry point against entry point to the bit; the guards that void an
iteration; the union step's capacity; and the argument refusals.

Every pointer handed to a kernel is a live device tensor of at least the size the call can reach and every surfel index is
below N, also in the cases that probe a capacity: buffers are sized by `capacity`, not by the union."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref
from adam_ref import BETAS, EPSS, LRS, STEPS, WIDTHS, Worst

pytestmark = pytest.mark.gpu

CONFIGS = [(b, e) for b in BETAS for e in EPSS]
DEFAULT = (BETAS[0], EPSS[0])


def _lib():
    from splat_loam_amd import _abi
    return _abi, _abi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _up(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _down(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# adam_kernel: sls_adam_step / _guarded / _reduced over groups of (param, grad, exp_avg, exp_avg_sq, lr)
# ---------------------------------------------------------------------------------------------------------------------
def _group_array(_abi, items):
    arr = (_abi.SlsAdamGroup * len(items))()
    for k, (p, g, m, v, lr) in enumerate(items):
        assert p.numel() == g.numel() == m.numel() == v.numel()
        assert all(x.dtype == torch.float32 and x.is_cuda and x.is_contiguous() for x in (p, g, m, v))
        arr[k].param, arr[k].grad, arr[k].exp_avg, arr[k].exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        arr[k].numel, arr[k].lr = p.numel(), lr
    return arr


def _adam(items, betas, eps, t, entry="step", skip=None, void=None, status=None, mirror=None):
    """One call of adam_kernel through `entry`; returns the return code, the stream drained."""
    _abi, lib = _lib()
    arr = _group_array(_abi, items)
    head = (arr, len(items), float(betas[0]), float(betas[1]), float(eps), int(t))
    if entry == "step":
        rc = lib.sls_adam_step(*head, _stream())
    elif entry == "guarded":
        rc = lib.sls_adam_step_guarded(*head, skip.data_ptr(), _stream())
    else:
        assert entry == "reduced"
        rc = lib.sls_adam_step_reduced(*head, void.data_ptr(), status.data_ptr() if status is not None else None,
                                       mirror.data_ptr() if mirror is not None else None, _stream())
    torch.cuda.synchronize()
    return rc


def _ok(rc, what):
    _abi, _ = _lib()
    _abi.check(rc, what)


def _chain_groups(device, sizes, lrs, configs, worst, what, seed, entry="step", **kw):
    """The shared inputs through the chained steps, one call per step over all groups; every element against its bounds."""
    for betas, eps in configs:
        rng = np.random.default_rng(seed)
        P = [_up(adam_ref.make_params(rng, n), device) for n in sizes]
        M = [torch.zeros(n, device=device) for n in sizes]
        V = [torch.zeros(n, device=device) for n in sizes]
        for t in STEPS:
            g = [adam_ref.make_grads(rng, n) for n in sizes]
            G = [_up(x, device) for x in g]
            before = [(_down(p), _down(m), _down(v)) for p, m, v in zip(P, M, V)]
            _ok(_adam(list(zip(P, G, M, V, lrs)), betas, eps, t, entry, **kw), f"sls_adam_{entry}")
            for k, n in enumerate(sizes):
                assert _same_bits(_down(G[k]), g[k]), "the gradient is an input"
                worst.check(f"{what} group {k} ({n})", before[k], g[k], (_down(P[k]), _down(M[k]), _down(V[k])), lrs[k],
                            betas[0], betas[1], eps, t)


def _lrs(n):
    return [LRS[k % 4] for k in range(n)]


def test_adam_step_group_sizes(device):
    """(a) numel 1 .. 5 (the scalar tail of a group alone), 1001 and 4004: each alone in a call and all in one call."""
    worst = Worst("sls_adam_step, group sizes")
    sizes = [1, 2, 3, 4, 5, 1001, 4004]
    _chain_groups(device, sizes, _lrs(7), CONFIGS, worst, "seven groups", seed=100)
    for k, n in enumerate(sizes):
        _chain_groups(device, [n], [LRS[k % 4]], [CONFIGS[k % 6]], worst, "alone", seed=200 + k)
    print(f"\n{worst}")


def test_adam_step_eight_groups_with_empty_ones(device):
    """(b) eight groups, the first, a middle one and the last of zero elements (their pointers are null, as an empty
    tensor's are): a unit's group is found by counting the prefix ends it has passed, and an empty group's end equals its
    predecessor's."""
    worst = Worst("sls_adam_step, eight groups")
    sizes = [0, 5, 1001, 7, 0, 4004, 3, 0]
    assert torch.empty(0, device=device).data_ptr() == 0
    _chain_groups(device, sizes, _lrs(8), CONFIGS, worst, "eight groups", seed=300)
    print(f"\n{worst}")


def test_adam_step_grid_stride(device):
    """(c) adam_kernel launches at most 2048 blocks of 256 threads, a unit of four elements per thread, and strides beyond
    that: 524 288 units a sweep.  Groups of 1 500 001 and 600 002 elements are 375 001 + 150 001 = 525 002 units: the group
    boundary (unit 375 001) is crossed inside the first sweep, and the second sweep — units 524 288 .. 525 001, 714 of them,
    the scalar tail of the second group included — lies wholly in the second group, so its threads look their group up
    afresh with a unit index beyond the grid.  A loop that ran once would leave the last 2 854 elements untouched."""
    worst = Worst("sls_adam_step, grid-stride loop")
    sizes = [1_500_001, 600_002]
    units = [(n + 3) // 4 for n in sizes]
    assert units == [375_001, 150_001] and units[0] < 2048 * 256 < sum(units)
    _chain_groups(device, sizes, [LRS[0], LRS[1]], [DEFAULT], worst, "two large groups", seed=400)
    print(f"\n{worst}")


def _one_step_state(rng, n):
    """A state as after a few steps: moments of the gradients' magnitudes."""
    return (adam_ref.make_params(rng, n), adam_ref.make_grads(rng, n), adam_ref.make_grads(rng, n) * np.float32(0.1),
            adam_ref.make_grads(rng, n) ** 2)


@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq"])
def test_adam_step_misaligned_pointer(device, which):
    """(d) one of the four pointers 1, 2 or 3 floats off a 16-byte boundary (a view into a larger tensor): the whole group
    takes the scalar path.  Same bits as the aligned call on the same values, and the floats on either side of the view
    keep their sentinel."""
    n, t, (betas, eps) = 1001, 3, DEFAULT
    rng = np.random.default_rng(500)
    host = dict(zip(("param", "grad", "exp_avg", "exp_avg_sq"), _one_step_state(rng, n)))
    aligned = {k: _up(a, device) for k, a in host.items()}
    assert all(x.data_ptr() % 16 == 0 for x in aligned.values())
    _ok(_adam([tuple(aligned.values()) + (LRS[2],)], betas, eps, t), "sls_adam_step")
    worst = Worst(f"sls_adam_step, aligned twin of the misaligned {which}")
    worst.check("aligned", (host["param"], host["exp_avg"], host["exp_avg_sq"]), host["grad"],
                tuple(_down(aligned[k]) for k in ("param", "exp_avg", "exp_avg_sq")), LRS[2], betas[0], betas[1], eps, t)
    sentinel = np.float32(-12345.678)
    for off in (1, 2, 3):
        dev = {k: _up(a, device) for k, a in host.items()}
        base = torch.full((n + 12,), float(sentinel), device=device)
        assert base.data_ptr() % 16 == 0
        lo = 4 + off
        base[lo:lo + n].copy_(dev[which])
        dev[which] = base[lo:lo + n]
        assert dev[which].data_ptr() % 16 == 4 * off and dev[which].is_contiguous()
        _ok(_adam([tuple(dev.values()) + (LRS[2],)], betas, eps, t), "sls_adam_step")
        for k in host:
            assert _same_bits(_down(dev[k]), _down(aligned[k])), f"{which} + {off} floats: {k} differs from the aligned call"
        edge = _down(base)
        assert (_bits(edge[:lo]) == _bits(sentinel)).all() and (_bits(edge[lo + n:]) == _bits(sentinel)).all(), \
            f"{which} + {off} floats: a float beside the view was written"


@pytest.mark.parametrize("betas,eps", CONFIGS)
def test_adam_step_zero_state_is_identity(device, betas, eps):
    """(e) g = 0, m = 0, v = 0: parameter and moments keep their bits (m * rcp(0 + eps) = 0 at both eps) — what every
    surfel no keyframe has reached yet relies on.  Among elements that do move, and past a float4 boundary."""
    rng = np.random.default_rng(600)
    n = 1003
    still = np.zeros(n, bool)
    still[[0, 1, 5, 6, 7, 8, 500, 1000, 1001, 1002]] = True
    for t in (1, 1000):
        p, g, m, v = _one_step_state(rng, n)
        p[0], p[1] = np.float32(-0.0), np.float32(1e-30)
        g[still], m[still], v[still] = 0.0, 0.0, 0.0
        P, G, M, V = (_up(x, device) for x in (p, g, m, v))
        _ok(_adam([(P, G, M, V, LRS[1])], betas, eps, t), "sls_adam_step")
        assert _same_bits(_down(P)[still], p[still])
        assert not _bits(_down(M)[still]).any() and not _bits(_down(V)[still]).any()
        assert not _same_bits(_down(P)[~still], p[~still])


@pytest.mark.parametrize("betas,eps", [DEFAULT, (BETAS[1], EPSS[1])])
def test_fused_adam_eleven_tensors(device, betas, eps, monkeypatch):
    """(f) FusedAdam hands sls_adam_step at most eight tensors a launch: eleven take two (8 + 3).  All eleven inside the
    bounds at every chained step, and state["step"] counts."""
    from splat_loam_amd import _abi
    from splat_loam_amd.optim import FusedAdam
    real = _abi.lib()

    class Counting:
        calls = []

        def __getattr__(self, name):
            return getattr(real, name)

        def sls_adam_step(self, arr, ngroups, *rest):
            self.calls.append(int(ngroups))
            return real.sls_adam_step(arr, ngroups, *rest)

    monkeypatch.setattr(_abi, "lib", lambda: Counting())
    shapes = [(1001, 3), (1001, 1), (1001, 2), (1001, 4), (5,), (1,), (4004,), (3,), (2,), (17, 3), (4,)]
    rng = np.random.default_rng(700)
    params = [_up(adam_ref.make_params(rng, int(np.prod(s))).reshape(s), device).requires_grad_(True) for s in shapes]
    lrs = _lrs(len(shapes))
    opt = FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(params, lrs)], lr=0.0, betas=betas, eps=eps)
    worst = Worst("FusedAdam, 11 tensors in two launches")
    for t in STEPS:
        if t == 1000:
            for p in params:
                opt.state[p]["step"] = 999
        g = [adam_ref.make_grads(rng, int(np.prod(s))).reshape(s) for s in shapes]
        before = []
        for p, x in zip(params, g):
            p.grad = _up(x, device)
            st = opt.state[p]
            zero = np.zeros(p.shape, np.float32)
            before.append((_down(p), _down(st["exp_avg"]) if len(st) else zero, _down(st["exp_avg_sq"]) if len(st) else zero))
        Counting.calls.clear()
        opt.step()
        torch.cuda.synchronize()
        assert Counting.calls == [8, 3]
        for k, p in enumerate(params):
            st = opt.state[p]
            assert int(st["step"]) == t
            worst.check(f"tensor {k} {shapes[k]}", before[k], g[k], (_down(p), _down(st["exp_avg"]), _down(st["exp_avg_sq"])),
                        lrs[k], betas[0], betas[1], eps, t)
    print(f"\n{worst}")


# ---------------------------------------------------------------------------------------------------------------------
# the model of N surfels: four parameter tensors and flat moment buckets [xyz 3N | opacity N | scaling 2N | rotation 4N]
# ---------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, N, flat_p, flat_m, flat_v, device):
        self.N, self.device = N, device
        edges = np.cumsum([0] + [w * N for w in WIDTHS])
        self.params = [_up(flat_p[a:b].reshape(N, w), device) for a, b, w in zip(edges[:-1], edges[1:], WIDTHS)]
        self.M, self.V = _up(flat_m, device), _up(flat_v, device)
        self.edges = edges

    def clone(self):
        return Model(self.N, *self.state(), self.device)

    def state(self):
        """(p, m, v) as flat float32 buckets of 10 N."""
        return np.concatenate([_down(p).ravel() for p in self.params]), _down(self.M), _down(self.V)

    def groups(self, flat_grad):
        """The model as four groups of sls_adam_step (moments and gradient: the blocks copied out of the flat buckets;
        write_back returns the moments)."""
        self._gm = [self.M[a:b].clone() for a, b in zip(self.edges[:-1], self.edges[1:])]
        self._gv = [self.V[a:b].clone() for a, b in zip(self.edges[:-1], self.edges[1:])]
        self._gg = [_up(flat_grad[a:b], self.device) for a, b in zip(self.edges[:-1], self.edges[1:])]
        return [(p.view(-1), g, m, v, lr) for p, g, m, v, lr in zip(self.params, self._gg, self._gm, self._gv, LRS)]

    def write_back(self):
        for a, b, m, v in zip(self.edges[:-1], self.edges[1:], self._gm, self._gv):
            self.M[a:b].copy_(m)
            self.V[a:b].copy_(v)


def _random_model(rng, N, device, stepped=True):
    n = 10 * N
    if stepped:
        p, _, m, v = _one_step_state(rng, n)
    else:
        p, m, v = adam_ref.make_params(rng, n), np.zeros(n, np.float32), np.zeros(n, np.float32)
    return Model(N, p, m, v, device)


def _status(device, words=(0,) * 8):
    return torch.tensor(list(words), dtype=torch.int32, device=device)


def _exchange(N, bits, flat_grad, device, capacity=None):
    """sls_grad_compact on ONE rank's bitmap: the union bitmap, its prefix, the union's rows and the status block."""
    _abi, lib = _lib()
    nw = int(lib.sls_grad_bitmap_words(N))
    K = int(np.count_nonzero(bits))
    cap = max(K, 1) if capacity is None else capacity
    out = dict(K=K, capacity=cap,
               maps=_up(adam_ref.pack_bitmap(N, bits, nw).view(np.int64), device),
               union=torch.zeros(nw, dtype=torch.int64, device=device),
               prefix=torch.zeros(nw, dtype=torch.int32, device=device),
               compact=torch.full(((max(cap, K) + 1) * 10,), -777.0, device=device),
               grads=_up(flat_grad, device), status=_status(device))
    _ok(lib.sls_grad_compact(N, out["maps"].data_ptr(), 1, out["union"].data_ptr(), out["grads"].data_ptr(),
                             out["compact"].data_ptr(), cap, out["prefix"].data_ptr(), out["status"].data_ptr(), _stream()),
        "sls_grad_compact")
    torch.cuda.synchronize()
    st = _down(out["status"])
    assert int(st[7]) == K and int(st[1]) == (4 if K > cap else 0)
    return out


def _sparse(model, ex, betas, eps, t, part, status=None, mirror=None):
    _, lib = _lib()
    status = ex["status"] if status is None else status
    rc = lib.sls_adam_step_sparse(model.N, *(p.data_ptr() for p in model.params), ex["union"].data_ptr(), ex["prefix"].data_ptr(),
                                  ex["compact"].data_ptr(), model.M.data_ptr(), model.V.data_ptr(), *LRS, float(betas[0]),
                                  float(betas[1]), float(eps), int(t), int(part), status.data_ptr(),
                                  mirror.data_ptr() if mirror is not None else None, _stream())
    torch.cuda.synchronize()
    return rc


def _union(model, index, compact, capacity, betas, eps, t, status, mirror=None):
    _, lib = _lib()
    assert index.dtype == torch.int32 and index.numel() >= capacity and compact.numel() >= 10 * capacity
    assert index.numel() == 0 or (0 <= int(index.min()) and int(index.max()) < model.N)
    rc = lib.sls_adam_step_union(model.N, *(p.data_ptr() for p in model.params), index.data_ptr(), compact.data_ptr(), capacity,
                                 model.M.data_ptr(), model.V.data_ptr(), *LRS, float(betas[0]), float(betas[1]), float(eps),
                                 int(t), status.data_ptr(), mirror.data_ptr() if mirror is not None else None, _stream())
    torch.cuda.synchronize()
    return rc


def _union_gradient(rng, N, bits):
    """A flat gradient bucket, zero outside the union."""
    rows = adam_ref.surfel_rows(N, adam_ref.make_grads(rng, 10 * N))
    rows[~np.asarray(bits, bool)] = 0.0
    return adam_ref.flat_from_rows(N, rows)


def _assert_same_state(a, b, what):
    for x, y, k in zip(a.state(), b.state(), ("parameters", "exp_avg", "exp_avg_sq")):
        if not _same_bits(x, y):
            i = int(np.flatnonzero(_bits(x) != _bits(y))[0])
            pytest.fail(f"{what}: {k} differ in {int((_bits(x) != _bits(y)).sum())} of {x.size} elements, e.g. [{i}] {x[i]!r} vs {y[i]!r}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. sls_adam_step_sparse against float64
# ---------------------------------------------------------------------------------------------------------------------
SPARSE_WORST = Worst("sls_grad_compact + sls_adam_step_sparse(part 0)")


@pytest.mark.parametrize("density", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 5000])
def test_adam_step_sparse_against_float64(device, N, density):
    """The flat-bucket exchange on one rank: sls_grad_compact packs the union's rows out of a flat gradient bucket whose
    rows OUTSIDE the union hold junk (the update must take zero there), sls_adam_step_sparse(part 0) updates all 10 N
    elements — three chained steps, a fresh union each.  A surfel outside the union takes the zero-gradient update: its
    moments decay and it moves by the decayed first moment."""
    worst = Worst(f"sls_adam_step_sparse N {N} density {density}")
    lr = adam_ref.flat_lr(N)
    for betas, eps in CONFIGS:
        rng = np.random.default_rng(1000 + N)
        model = _random_model(rng, N, device, stepped=False)
        for t in (1, 2, 3):
            bits = rng.random(N) < density if 0.0 < density < 1.0 else np.full(N, density == 1.0)
            junk = adam_ref.make_grads(rng, 10 * N)
            rows = adam_ref.surfel_rows(N, junk)
            rows[~bits] = 0.0
            g = adam_ref.flat_from_rows(N, rows)
            ex = _exchange(N, bits, junk, device)
            before = model.state()
            _ok(_sparse(model, ex, betas, eps, t, part=0), "sls_adam_step_sparse")
            for w in (worst, SPARSE_WORST):
                w.check(f"N {N} density {density}", before, g, model.state(), lr, betas[0], betas[1], eps, t)
    print(f"\n{worst}\n{SPARSE_WORST} so far")


# ---------------------------------------------------------------------------------------------------------------------
# same bits through every entry point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas,eps", CONFIGS)
@pytest.mark.parametrize("N", [257, 5000])
def test_every_entry_point_gives_the_same_bits(device, N, betas, eps):
    """The comment above AdamCoef promises one set of bits whichever kernel applies the update, and the sparse exchange's
    "every rank ends with the all-reduce path's parameters" rests on it.  Same operands, integer views.  (Each side is
    inside the float64 bounds by the other tests; a difference here alone means the compiler contracted adam_one's
    multiply-adds differently in two kernels.)"""
    t = 3
    rng = np.random.default_rng(2000 + N)
    start = _random_model(rng, N, device)
    bits = rng.random(N) < 0.3
    g = _union_gradient(rng, N, bits)

    plain = start.clone()
    _ok(_adam(plain.groups(g), betas, eps, t), "sls_adam_step")
    plain.write_back()
    worst = Worst("sls_adam_step on the model's four tensors")
    worst.check(f"N {N}", start.state(), g, plain.state(), adam_ref.flat_lr(N), betas[0], betas[1], eps, t)

    guarded = start.clone()
    _ok(_adam(guarded.groups(g), betas, eps, t, "guarded", skip=_status(device, (0,))), "sls_adam_step_guarded")
    guarded.write_back()
    _assert_same_state(guarded, plain, "sls_adam_step_guarded(*skip_flag = 0) vs sls_adam_step")

    reduced = start.clone()
    status, mirror = _status(device, (9, 7, 1, 2, 3, 4, 5, 6)), _status(device, (-1,) * 8)
    _ok(_adam(reduced.groups(g), betas, eps, t, "reduced", void=torch.zeros(2, device=device), status=status, mirror=mirror),
        "sls_adam_step_reduced")
    reduced.write_back()
    _assert_same_state(reduced, plain, "sls_adam_step_reduced(void_flags = (0, 0)) vs sls_adam_step")
    assert _down(status).tolist() == [9, 0, 1, 2, 3, 4, 5, 6] and _down(mirror).tolist() == [9, 0, 1, 2, 3, 4, 5, 6]

    ex = _exchange(N, bits, g, device)
    sparse0 = start.clone()
    _ok(_sparse(sparse0, ex, betas, eps, t, part=0), "sls_adam_step_sparse")
    _assert_same_state(sparse0, plain, "sls_adam_step_sparse(part 0) vs sls_adam_step on the rows scattered back")

    outside = start.clone()
    _ok(_sparse(outside, ex, betas, eps, t, part=1), "sls_adam_step_sparse")
    sparse12 = outside.clone()
    _ok(_sparse(sparse12, ex, betas, eps, t, part=2), "sls_adam_step_sparse")
    _assert_same_state(sparse12, sparse0, "sls_adam_step_sparse part 1 then part 2 vs part 0")
    # ... and each part kept to its side of the union
    in_union = np.concatenate([np.repeat(bits, w) for w in WIDTHS])
    for x, y, z in zip(outside.state(), start.state(), sparse0.state()):
        assert _same_bits(x[in_union], y[in_union]) and _same_bits(x[~in_union], z[~in_union])

    union = outside.clone()
    index = _up(np.flatnonzero(bits).astype(np.int32), device)
    status = _status(device, (0,) * 7 + (ex["K"],))
    _ok(_union(union, index, ex["compact"], ex["K"], betas, eps, t, status), "sls_adam_step_union")
    _assert_same_state(union, sparse12, "sls_adam_step_union vs sls_adam_step_sparse(part 2)")


# ---------------------------------------------------------------------------------------------------------------------
# guards: a void iteration changes nothing and still reports
# ---------------------------------------------------------------------------------------------------------------------
def _assert_untouched(model, start, what):
    for x, y in zip(model.state(), start):
        assert _same_bits(x, y), f"{what}: a void iteration wrote parameters or moments"


def test_guarded_and_reduced_skip_a_void_iteration(device):
    N, t, (betas, eps) = 257, 2, DEFAULT
    rng = np.random.default_rng(3000)
    model = _random_model(rng, N, device)
    start = model.state()
    g = adam_ref.make_grads(rng, 10 * N)
    for flag in (1, 4, -2**31):
        _ok(_adam(model.groups(g), betas, eps, t, "guarded", skip=_status(device, (flag,))), "sls_adam_step_guarded")
        model.write_back()
        _assert_untouched(model, start, f"sls_adam_step_guarded, skip flag {flag}")
    block = (9, 77, 1, 2, 3, 4, 5, 6)
    for flags, verdict in (((3.0, 0.0), 1), ((0.0, 1.0), 2), ((2.0, 5.0), 3)):
        void = torch.tensor(flags, device=device)
        # the mirror is the host-visible copy in production; any 8 device words serve
        status, mirror = _status(device, block), _status(device, (-1,) * 8)
        _ok(_adam(model.groups(g), betas, eps, t, "reduced", void=void, status=status, mirror=mirror), "sls_adam_step_reduced")
        model.write_back()
        _assert_untouched(model, start, f"sls_adam_step_reduced, void flags {flags}")
        want = [block[0], verdict] + list(block[2:])
        assert _down(status).tolist() == want and _down(mirror).tolist() == want, (flags, _down(status), _down(mirror))
        # no units at all (every group empty): the verdict is still published
        status, mirror = _status(device, block), _status(device, (-1,) * 8)
        empty = torch.empty(0, device=device)
        _ok(_adam([(empty, empty, empty, empty, LRS[0])] * 2, betas, eps, t, "reduced", void=void, status=status, mirror=mirror),
            "sls_adam_step_reduced")
        assert _down(status).tolist() == want and _down(mirror).tolist() == want, (flags, _down(status), _down(mirror))
        # ... and without a status block there is nothing to publish and nothing is updated
        _ok(_adam(model.groups(g), betas, eps, t, "reduced", void=void), "sls_adam_step_reduced")
        model.write_back()
        _assert_untouched(model, start, f"sls_adam_step_reduced without a status block, void flags {flags}")
    # an iteration that is not void, no units: the mirror carries the block with verdict 0
    status, mirror = _status(device, block), _status(device, (-1,) * 8)
    empty = torch.empty(0, device=device)
    _ok(_adam([(empty, empty, empty, empty, LRS[0])], betas, eps, t, "reduced", void=torch.zeros(2, device=device), status=status,
              mirror=mirror), "sls_adam_step_reduced")
    assert _down(mirror).tolist() == [block[0], 0] + list(block[2:]) == _down(status).tolist()


@pytest.mark.parametrize("overflow", [1, 2, 4, 32])
def test_sparse_and_union_skip_a_void_iteration(device, overflow):
    """status[1] != 0 — the group's verdict or an exchange buffer too small: no surfel is updated by any part, and the
    parts that close the iteration (0, 2, the union step) mirror the status block as it stands; part 1 never does."""
    N, t, (betas, eps) = 257, 2, DEFAULT
    rng = np.random.default_rng(3100)
    model = _random_model(rng, N, device)
    start = model.state()
    bits = rng.random(N) < 0.3
    ex = _exchange(N, bits, _union_gradient(rng, N, bits), device)
    block = (9, overflow, 1, 2, 3, 4, 5, ex["K"])
    index = _up(np.flatnonzero(bits).astype(np.int32), device)
    for what in ("part 0", "part 1", "part 2", "union"):
        status, mirror = _status(device, block), _status(device, (-1,) * 8)
        if what == "union":
            _ok(_union(model, index, ex["compact"], ex["K"], betas, eps, t, status, mirror), "sls_adam_step_union")
        else:
            _ok(_sparse(model, ex, betas, eps, t, int(what[-1]), status, mirror), "sls_adam_step_sparse")
        _assert_untouched(model, start, f"{what}, status[1] = {overflow}")
        assert _down(status).tolist() == list(block)
        assert _down(mirror).tolist() == ([-1] * 8 if what == "part 1" else list(block)), (what, _down(mirror))


def test_sparse_and_union_mirror_a_live_iteration(device):
    """The mirror of an iteration that is NOT void: parts 0 and 2 and the union step write it, part 1 does not, and a null
    mirror is accepted."""
    N, t, (betas, eps) = 65, 1, DEFAULT
    rng = np.random.default_rng(3200)
    bits = rng.random(N) < 0.5
    ex = _exchange(N, bits, _union_gradient(rng, N, bits), device)
    block = (9, 0, 1, 2, 3, 4, 5, ex["K"])
    index = _up(np.flatnonzero(bits).astype(np.int32), device)
    for what in ("part 0", "part 1", "part 2", "union"):
        model = _random_model(rng, N, device)
        start = model.state()
        status, mirror = _status(device, block), _status(device, (-1,) * 8)
        if what == "union":
            _ok(_union(model, index, ex["compact"], ex["K"], betas, eps, t, status, mirror), "sls_adam_step_union")
        else:
            _ok(_sparse(model, ex, betas, eps, t, int(what[-1]), status, mirror), "sls_adam_step_sparse")
        assert _down(mirror).tolist() == ([-1] * 8 if what == "part 1" else list(block)), (what, _down(mirror))
        assert not _same_bits(model.state()[0], start[0])


# ---------------------------------------------------------------------------------------------------------------------
# sls_adam_step_union: capacity against the union's size
# ---------------------------------------------------------------------------------------------------------------------
UNION_WORST = Worst("sls_adam_step_union")


def _union_cases(N):
    """(K, capacity): K = 0, a middle K and K = N; capacity = K, K + 300 (needs a surfel outside the union for the slots
    past K) and K - 1 (a launch needs capacity >= 1)."""
    cases = []
    for K in sorted({0, N // 3, N}):
        for cap in (K, K + 300, K - 1):
            if cap >= 1 and not (cap > K and K == N):
                cases.append((K, cap))
    return cases


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 5000])
def test_adam_step_union_capacity(device, N):
    """The live slots are min(capacity, status.exchange_count): exactly the surfels index[: min(capacity, K)] are updated
    (inside the float64 bounds, row for row), every other surfel keeps its bits — the one whose index fills the slots
    past K included (a kernel that trusted `capacity` alone would update it with a junk row)."""
    t, (betas, eps) = 3, DEFAULT
    rng = np.random.default_rng(4000 + N)
    lr = adam_ref.flat_lr(N)
    assert _union_cases(N)
    for K, cap in _union_cases(N):
        model = _random_model(rng, N, device)
        before = model.state()
        order = rng.permutation(N)
        room = max(cap, K)
        index = np.empty(room, np.int32)
        index[:K] = order[:K]
        if room > K:
            index[K:] = order[K]                                 # a surfel that is NOT in the union
        rows = adam_ref.surfel_rows(room, adam_ref.make_grads(rng, 10 * room))
        rows[K:] = 1.0                                           # (what the slots past K would apply if they were read)
        live = min(cap, K)
        updated = np.zeros(N, bool)
        updated[index[:live]] = True
        g_rows = np.zeros((N, 10), np.float32)
        g_rows[index[:live]] = rows[:live]
        status = _status(device, (0,) * 7 + (K,))
        _ok(_union(model, _up(index, device), _up(rows.reshape(-1), device), cap, betas, eps, t, status), "sls_adam_step_union")
        after = model.state()
        elem = np.concatenate([np.repeat(updated, w) for w in WIDTHS])
        for x, y, what in zip(after, before, ("parameters", "exp_avg", "exp_avg_sq")):
            assert _same_bits(x[~elem], y[~elem]), f"N {N} K {K} capacity {cap}: {what} of a surfel outside index[:{live}] changed"
        if live:
            sel = [x[elem] for x in before], adam_ref.flat_from_rows(N, g_rows)[elem], [x[elem] for x in after]
            UNION_WORST.check(f"N {N} K {K} capacity {cap}", sel[0], sel[1], sel[2], lr[elem], betas[0], betas[1], eps, t)
            assert not _same_bits(after[2][elem], before[2][elem])
    print(f"\n{UNION_WORST} so far")


# ---------------------------------------------------------------------------------------------------------------------
# argument refusals: -1 and a message, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_refusals(device):
    _abi, lib = _lib()
    N, (betas, eps) = 65, DEFAULT
    rng = np.random.default_rng(5000)
    model = _random_model(rng, N, device)
    start = model.state()
    bits = rng.random(N) < 0.5
    g = _union_gradient(rng, N, bits)
    ex = _exchange(N, bits, g, device)
    index = _up(np.flatnonzero(bits).astype(np.int32), device)
    status = _status(device, (0,) * 7 + (ex["K"],))

    def refused(rc, word):
        assert rc == -1, rc
        msg = lib.sls_last_error().decode()
        assert word in msg, msg
        _assert_untouched(model, start, msg)

    refused(_sparse(model, ex, betas, eps, 1, part=3), "part")
    refused(_sparse(model, ex, betas, eps, 1, part=-1), "part")
    refused(_sparse(model, ex, betas, eps, 0, part=0), "step")
    refused(_union(model, index, ex["compact"], ex["K"], betas, eps, 0, status), "step")
    refused(_union(model, index, ex["compact"], 0, betas, eps, 1, status), "bad argument")
    for entry, kw in (("step", {}), ("guarded", dict(skip=_status(device, (0,)))),
                      ("reduced", dict(void=torch.zeros(2, device=device)))):
        refused(_adam(model.groups(g), betas, eps, 0, entry, **kw), "step")
    # the rows and the bucket they are packed from come together or not at all
    nw = int(lib.sls_grad_bitmap_words(N))
    union, prefix = torch.zeros(nw, dtype=torch.int64, device=device), torch.zeros(nw, dtype=torch.int32, device=device)
    head = (N, ex["maps"].data_ptr(), 1, union.data_ptr())
    tail = (ex["capacity"], prefix.data_ptr(), status.data_ptr(), _stream())
    refused(lib.sls_grad_compact(*head, ex["grads"].data_ptr(), None, *tail), "bad argument")
    refused(lib.sls_grad_compact(*head, None, ex["compact"].data_ptr(), *tail), "bad argument")
    torch.cuda.synchronize()
    assert not _down(union).any() and not _down(prefix).any() and _down(status).tolist() == [0] * 7 + [ex["K"]]
    # ... and the library still works
    _ok(_sparse(model, ex, betas, eps, 1, part=0), "sls_adam_step_sparse")
    assert not _same_bits(model.state()[0], start[0])
