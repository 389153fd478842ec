"""NumPy model of the depth-order repair (splat_loam_amd/csrc/sls_sort.hip, "Temporal re-sort of the depth order") on
(key, surfel) pairs packed as key << 32 | surfel — shared by tests/test_repair_local_rounds.py.

    window_sort      step A: aligned windows of 1024 positions of the OLD order, keyed anew and sorted
    global_rounds    k repair rounds as k launches over the whole order: 2k - 1 levels of window merges, shifted,
                     aligned, shifted, ... (a merge of two sorted halves is a sort of the window)
    local_rounds     the one-launch form: window b merges once, and only a window with an out-of-order boundary inside
                     its cone of dependence redoes the 2k - 1 levels on the 2k aligned windows around it
    verdict          step C: strictly increasing window edges <=> the exact order

Both forms pad the positions in front of the order with 0 and those behind its end with ~0, as the kernels do."""
import numpy as np

W = 1024
H = W // 2
PAD_HI = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack(keys_by_surfel, order):
    order = np.asarray(order, dtype=np.uint64)
    return (np.asarray(keys_by_surfel, dtype=np.uint64)[order.astype(np.int64)] << np.uint64(32)) | order


def window_sort(keys_by_surfel, prev_order):
    comp = pack(keys_by_surfel, prev_order)
    for a in range(0, comp.size, W):
        comp[a:a + W] = np.sort(comp[a:a + W])
    return comp


def n_shifted(N):
    return (N + H + W - 1) // W          # shifted windows that hold a real element


def _pairs_at(comp, lo, hi):
    """comp[lo:hi] with the padding on both sides of the order"""
    N = comp.size
    out = np.empty(hi - lo, dtype=np.uint64)
    pos = np.arange(lo, hi)
    out[pos < 0] = 0
    out[pos >= N] = PAD_HI
    real = (pos >= 0) & (pos < N)
    out[real] = comp[pos[real]]
    return out


def _levels(buf, k):
    """the 2k - 1 levels on a run of whole aligned windows, every window of every level (in place)"""
    n = buf.size // W
    for level in range(1, 2 * k):
        off = H if level & 1 else 0
        for w in range(n - (1 if off else 0)):
            buf[w * W + off:(w + 1) * W + off] = np.sort(buf[w * W + off:(w + 1) * W + off])


def verdict(out):
    """True: the edges of the shifted windows are strictly increasing (each window is sorted, so: the exact order)"""
    N = out.size
    ok = True
    for b in range(n_shifted(N) - 1):
        hi = min((b + 1) * W - H, N) - 1          # last real element of window b
        ok &= bool(out[hi] < out[hi + 1])         # first of window b + 1
    return ok


def global_rounds(comp, k):
    N = comp.size
    nA = (N + W - 1) // W
    buf = _pairs_at(comp, -W, (nA + 1) * W)
    _levels(buf, k)
    out = buf[W:W + N].copy()
    return out, verdict(out)


def boundary_in_order(comp, j):
    """boundary j lies between shifted windows j and j + 1 (after level 1), at position m; decided from the
    window-sorted pairs alone"""
    N = comp.size
    m = j * W + H
    if m <= 0 or m >= N:
        return True          # one side holds padding only
    at = lambda p: _pairs_at(comp, p, p + 1)[0]
    return bool(max(at(m - H - 1), at(m - 1)) < min(at(m), at(m + H)))


def _cone_levels(cone, k):
    """The 2k - 1 levels on the cone of an escalated window, each level one window fewer on either end, as the kernel
    runs them: a merge whose two (sorted) halves are already in order is skipped.  In place; -> the number of merges run."""
    n = 2 * k
    ran = 0
    for level in range(1, n):
        off = H if level & 1 else 0
        first = level >> 1
        last = n - 1 - first - (1 if off else 0)
        for w in range(first, last + 1):
            a = w * W + off
            if cone[a + H - 1] <= cone[a + H]:          # (equal: padding)
                continue
            cone[a:a + W] = np.sort(cone[a:a + W])
            ran += 1
    return ran


def local_rounds(comp, k):
    """-> (order of pairs, verdict, number of windows that escalated, merges they ran)"""
    N = comp.size
    out = np.empty(N, dtype=np.uint64)
    escalated = merges = 0
    for b in range(n_shifted(N)):
        lo, hi = b * W - H, b * W + H
        esc = k >= 2 and not all(boundary_in_order(comp, j) for j in range(b - k + 1, b + k - 1))
        if not esc:
            win = np.sort(_pairs_at(comp, lo, hi))
        else:
            escalated += 1
            cone = _pairs_at(comp, (b - k) * W, (b + k) * W)
            merges += _cone_levels(cone, k)
            win = cone[k * W - H:k * W + H]
        real = np.arange(lo, hi)
        keep = (real >= 0) & (real < N)
        out[real[keep]] = win[keep]
    return out, verdict(out), escalated, merges
