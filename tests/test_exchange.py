"""The touched-set exchange's device pieces alone (sls_exchange.hip): the OR of the ranks' bitmaps,
its exclusive bit-count prefix, the union's size and the group's verdict — against NumPy, at sizes that take every path of
the one-workgroup kernel (runs of odd and even length in LDS, the padded layout, models too large for LDS); and the rows
sls_grad_compact packs behind them, against tests/adam_ref.py's compact_rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,G", [(1, 1), (63, 2), (5000, 2), (65600, 3), (100000, 2), (500000, 8), (786432, 1), (1000001, 3)])
def test_grad_union_matches_numpy(device, N, G):
    from splat_loam_amd import _abi
    lib = _abi.lib()
    rng = np.random.default_rng(N + G)
    nw = int(lib.sls_grad_bitmap_words(N))
    assert nw == (N + 63) // 64 + 2
    maps = np.zeros((G, nw), np.uint64)
    for g in range(G):
        bits = rng.random(nw * 64 - 128) < (0.02 + 0.1 * g)
        bits[N:] = False                                     # (bits beyond N are never set by the producers)
        maps[g, :nw - 2] = np.packbits(bits, bitorder="little").view(np.uint64)
    maps[G - 1, nw - 1] = 1 if N % 2 else 0                  # one rank voids the iteration (bit 1 of the verdict) for odd N
    want = np.bitwise_or.reduce(maps, axis=0)
    counts = np.array([bin(int(w)).count("1") for w in want[:nw - 2]], np.int64)
    prefix = np.concatenate([[0], np.cumsum(counts)[:-1]])
    K = int(counts.sum())
    for cap in (max(K, 1), max(K - 1, 1)):
        d_maps = torch.tensor(maps.view(np.int64).reshape(-1), device=device)
        d_union = torch.full((nw,), -1, dtype=torch.int64, device=device)
        d_prefix = torch.full((nw,), -1, dtype=torch.int32, device=device)
        status = torch.zeros((8,), dtype=torch.int32, device=device)
        _abi.check(lib.sls_grad_union(N, d_maps.data_ptr(), G, d_union.data_ptr(), cap, d_prefix.data_ptr(), status.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "sls_grad_union")
        torch.cuda.synchronize()
        assert np.array_equal(d_union.cpu().numpy().view(np.uint64), want)
        assert np.array_equal(d_prefix.cpu().numpy()[:nw - 2].astype(np.int64), prefix)
        st = status.cpu().numpy()
        assert int(st[7]) == K
        assert int(st[1]) == (2 if N % 2 else 0) | (4 if K > cap else 0)


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 5000, 65600])
def test_grad_compact_rows_match_numpy(device, N, G):
    """sls_grad_compact's second kernel: the ten gradient values of every surfel of the union, in surfel order, out of the
    flat [xyz 3N | opacity N | scaling 2N | rotation 4N] bucket into compact[slot][10] — bit for bit the rows of
    adam_ref.compact_rows.  grads_flat[k] = k (exact below 2^24) names the element every value came from.  Capacities at,
    below and above the union's size: a row at or beyond `capacity` is never written (sentinels), K is reported as it is and
    bit 2 of the verdict rises exactly when K > capacity.  (65600 is the first size whose per-thread run of bitmap words is
    even: the padded LDS layout of the prefix kernel.)"""
    import adam_ref
    from splat_loam_amd import _abi
    lib = _abi.lib()
    assert 10 * N < 2 ** 24
    rng = np.random.default_rng(7 * N + G)
    nw = int(lib.sls_grad_bitmap_words(N))
    ranks = rng.random((G, N)) < (0.5 if N < 64 else 0.1)
    if N in (1, 63):
        ranks[0, [0, N - 1]] = True                            # the first and the last surfel of a word
    if N == 257:
        ranks[0, [63, 64, 255, 256]] = True                  # ... and both sides of two word boundaries
    maps = np.stack([adam_ref.pack_bitmap(N, r, nw) for r in ranks])
    bits = ranks.any(axis=0)
    K = int(bits.sum())
    flat = np.arange(10 * N, dtype=np.float32)
    want = adam_ref.compact_rows(N, bits, flat)
    d_maps = torch.tensor(maps.view(np.int64).reshape(-1), device=device)
    d_flat = torch.tensor(flat, device=device)
    for cap in sorted({c for c in (K, K - 1, K + 7) if c >= 1}):
        rows = max(K, cap) + 1
        d_union = torch.full((nw,), -1, dtype=torch.int64, device=device)
        d_prefix = torch.full((nw,), -1, dtype=torch.int32, device=device)
        d_compact = torch.full((rows, 10), -1.0, device=device)
        status = torch.zeros((8,), dtype=torch.int32, device=device)
        _abi.check(lib.sls_grad_compact(N, d_maps.data_ptr(), G, d_union.data_ptr(), d_flat.data_ptr(), d_compact.data_ptr(), cap,
                                        d_prefix.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "sls_grad_compact")
        torch.cuda.synchronize()
        got = d_compact.cpu().numpy()
        live = min(K, cap)
        assert np.array_equal(got[:live].view(np.uint32), want[:live].view(np.uint32)), (N, G, cap)
        assert (got[live:] == -1.0).all(), f"N {N} G {G}: a row at or beyond capacity {cap} was written (K = {K})"
        assert np.array_equal(d_union.cpu().numpy()[:nw - 2].view(np.uint64), adam_ref.pack_bitmap(N, bits, nw)[:nw - 2])
        st = status.cpu().numpy()
        assert int(st[7]) == K
        assert int(st[1]) == (4 if K > cap else 0)
        assert np.array_equal(d_flat.cpu().numpy(), flat)
