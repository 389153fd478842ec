"""include/sls_outlier_math.h on the host, as plain C99 — the very list insertion, mean and keep rules the kernels run —
against the NumPy restatement (outlier_ref.py), and the restatement itself on cases worked by hand and against a KD-tree."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import outlier_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_NONE = outlier_ref.KEY_NONE

PROGRAM = r'''
#include <stdio.h>
#include <stdlib.h>
#include "sls_outlier_math.h"
/* lists: [K, k, Mt, streams, length] int32, then streams x length keys -> per stream K keys and the mean of its k-list,
 *        built as the kernel builds it: K - k slots of 0 in front, the rest SLS_NN_KEY_NONE, a guarded insertion per key
 * rules: [M, 0, 0, 0, 0] int32, std_ratio, thr_in (doubles), radius (float, padded to 8 bytes), M means (doubles), M keys
 *        -> cloud_mean, std, thr (doubles, sequential sums), then per point: counts, keep(thr), keep(thr_in), radius keep */
int main(int argc, char **argv) {
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    int h[5];
    if (fread(h, 4, 5, in) != 5) return 2;
    if (argv[1][0] == 'l') {
        const int K = h[0], k = h[1], Mt = h[2], first = K - k;
        uint64_t list[SLS_NN_K_MAX], key;
        if (sls_knn_list_length(k) != K) return 3;
        for (int s = 0; s < h[3]; ++s) {
            for (int j = 0; j < K; ++j) list[j] = j < first ? 0ull : SLS_NN_KEY_NONE;
            for (int i = 0; i < h[4]; ++i) {
                if (fread(&key, 8, 1, in) != 1) return 2;
                if (key < list[K - 1]) sls_knn_insert(list, K, key);
            }
            const double mean = sls_knn_mean(list, K, first, k < Mt ? k : Mt);
            fwrite(list, 8, (size_t)K, out); fwrite(&mean, 8, 1, out);
        }
    } else {
        const int M = h[0];
        double par[3], *mean = malloc(8 * (size_t)M), sum = 0.0, dev2 = 0.0;
        uint64_t *key = malloc(8 * (size_t)M);
        if (fread(par, 8, 3, in) != 3 || fread(mean, 8, (size_t)M, in) != (size_t)M || fread(key, 8, (size_t)M, in) != (size_t)M) return 2;
        float radius;
        __builtin_memcpy(&radius, &par[2], 4);
        for (int i = 0; i < M; ++i) if (sls_outlier_counts(mean[i])) sum += mean[i];
        const double cm = sls_outlier_cloud_mean(sum, M);
        for (int i = 0; i < M; ++i) if (sls_outlier_counts(mean[i])) dev2 += sls_outlier_dev2(mean[i], cm);
        const double sd = sls_outlier_std(dev2, M), thr = sls_outlier_threshold(cm, sd, par[0]);
        fwrite(&cm, 8, 1, out); fwrite(&sd, 8, 1, out); fwrite(&thr, 8, 1, out);
        for (int i = 0; i < M; ++i) {
            const unsigned char f[4] = { (unsigned char)sls_outlier_counts(mean[i]), (unsigned char)sls_outlier_keep_statistical(mean[i], thr),
                                         (unsigned char)sls_outlier_keep_statistical(mean[i], par[1]),
                                         (unsigned char)sls_outlier_keep_radius(key[i], radius) };
            fwrite(f, 1, 4, out);
        }
        free(mean); free(key);
    }
    fclose(in); fclose(out);
    return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    d = tmp_path_factory.mktemp("outlier_math")
    (d / "outlier_math.c").write_text(PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           str(d / "outlier_math.c"), "-o", str(d / "outlier_math"), "-lm"])
    return str(d / "outlier_math")


def run_lists(exe, tmp_path, K, k, Mt, keys):
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([K, k, Mt, keys.shape[0], keys.shape[1]], np.int32).tobytes())
        f.write(np.ascontiguousarray(keys, np.uint64).tobytes())
    subprocess.check_call([exe, "lists", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    got = np.fromfile(tmp_path / "out.bin", np.uint64).reshape(keys.shape[0], K + 1)
    return got[:, :K], got[:, K].copy().view(np.float64)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 9, 16, 17, 20, 32])
def test_list_insertion_against_a_sort(exe, tmp_path, k):
    """Random key streams with many equal distances (6 distinct ones, among them 0 and, for target 0, the key 0 itself)
    and as many targets as the stream is long, each once: the list is the sorted stream's head, behind K - k zeros."""
    rng = np.random.default_rng(k)
    K = next(v for v in (4, 8, 16, 32) if v >= k)
    for length in (0, 1, k - 1, k, k + 1, 200):
        if length < 0:
            continue
        d2 = rng.choice(np.array([0.0, 0.00390625, 0.25, 1.0, 1.00390625, 4096.0], np.float32), (50, length))
        idx = np.argsort(rng.random((50, length)), axis=1).astype(np.uint64)           # every target index once, any order
        keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx
        lists, mean = run_lists(exe, tmp_path, K, k, length, keys)
        want = np.full((50, k), KEY_NONE, np.uint64)
        n = min(k, length)
        want[:, :n] = np.sort(keys, axis=1)[:, :n]
        assert np.all(lists[:, :K - k] == 0) and np.array_equal(lists[:, K - k:], want), (k, length)
        if n:
            assert np.array_equal(mean.view(np.uint64), outlier_ref.means(want, length).view(np.uint64)), (k, length)


def run_rules(exe, tmp_path, mean, keys, std_ratio, thr_in, radius):
    par = np.zeros(3, np.float64)
    par[0], par[1] = std_ratio, thr_in
    par[2:3].view(np.float32)[0] = radius
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(mean), 0, 0, 0, 0], np.int32).tobytes())
        f.write(par.tobytes() + np.ascontiguousarray(mean, np.float64).tobytes() + np.ascontiguousarray(keys, np.uint64).tobytes())
    subprocess.check_call([exe, "rules", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    raw = open(tmp_path / "out.bin", "rb").read()
    return np.frombuffer(raw[:24], np.float64), np.frombuffer(raw[24:], np.uint8).reshape(-1, 4)


@pytest.mark.parametrize("M,k", [(63, 2), (257, 3), (1500, 20), (3000, 32), (1, 3), (40, 1)])
def test_means_and_keep_rules_bit_for_bit(exe, tmp_path, M, k):
    pts = outlier_ref.filter_cloud(M, 7 * M + k) if M > 10 else np.zeros((M, 3), np.float32)
    ref = outlier_ref.statistical(pts, k, 2.0)
    radius = 0.4330127
    rank = outlier_ref.keys_k(pts, pts, 4)[:, 3]
    (cm, sd, thr), flags = run_rules(exe, tmp_path, ref["mean"], rank, 2.0, ref["thr"], radius)
    assert np.array_equal(flags[:, 0] != 0, ref["mean"] > 0)
    assert np.array_equal(flags[:, 2] != 0, ref["keep"])                      # the rule itself, at the restatement's threshold
    assert np.array_equal(flags[:, 3] != 0, outlier_ref.radius(pts, 3, radius))
    if M > 1 and k > 1:
        for got, want in ((cm, ref["cloud_mean"]), (sd, ref["std"]), (thr, ref["thr"])):
            assert abs(got - want) <= 1e-12 * abs(want)                         # (sequential sums here, pairwise in NumPy)
        assert ref["margin"] > 1e-6 and np.array_equal(flags[:, 1] != 0, ref["keep"])
        assert 0 < ref["keep"].sum() < M
    else:
        assert not flags[:, 1].any() and not ref["keep"].any()                  # M = 1: thr is NaN; k = 1: every mean is 0
        assert np.isnan(thr) == (M == 1)


def test_restatement_worked_by_hand():
    # five points on a line, an exact copy, one far point
    pts = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [3, 0, 0], [0, 0.5, 0], [100, 0, 0]], np.float32)
    d2, idx = outlier_ref.nearest_k(pts, pts, 3)
    assert idx.tolist() == [[0, 4, 1], [1, 2, 0], [1, 2, 0], [3, 1, 2], [4, 0, 1], [5, 3, 1]]       # lower index first at equal d2
    assert d2.tolist() == [[0, 0.25, 1], [0, 0, 1], [0, 0, 1], [0, 4, 4], [0, 0.25, 1.25], [0, 97 * 97, 99 * 99]]
    mean = outlier_ref.means(outlier_ref.keys_k(pts, pts, 3), 6)
    r125 = float(np.sqrt(np.float32(1.25)))
    assert mean.tolist() == [1.5 / 3, 1.0 / 3, 1.0 / 3, 4.0 / 3, (0.5 + r125) / 3, 196.0 / 3]
    st = outlier_ref.statistical(pts, 3, 1.0)
    cm = mean.sum() / 6
    sd = np.sqrt(((mean - cm) ** 2).sum() / 5)
    assert st["zero_mean"] == 0 and abs(st["cloud_mean"] - cm) < 1e-15 and abs(st["thr"] - (cm + sd)) < 1e-13
    assert st["keep"].tolist() == [True, True, True, True, True, False]
    # k = 2: the two copies have a zero mean, do not enter the sums and are removed; n stays M
    st = outlier_ref.statistical(pts, 2, 1.0)
    m2 = np.array([0.25, 0, 0, 1.0, 0.25, 48.5])
    assert st["mean"].tolist() == m2.tolist() and st["zero_mean"] == 2
    assert abs(st["cloud_mean"] - 50.0 / 6) < 1e-15
    assert abs(st["std"] - np.sqrt((((m2 - 50.0 / 6) ** 2)[m2 > 0]).sum() / 5)) < 1e-13
    assert st["keep"].tolist() == [True, False, False, True, True, False]
    # k = 1 removes everything; M = 1 removes the point; M < k: the mean is over the M entries there are
    assert not outlier_ref.statistical(pts, 1, 2.0)["keep"].any() and outlier_ref.statistical(pts, 1, 2.0)["zero_mean"] == 6
    one = outlier_ref.statistical(pts[:1], 3, 2.0)
    assert one["keep"].tolist() == [False] and np.isnan(one["thr"])
    keys = outlier_ref.keys_k(pts[:2], pts[:2], 4)
    assert (keys[:, 2:] == KEY_NONE).all() and outlier_ref.split(keys)[1].tolist() == [[0, 1, -1, -1], [1, 0, -1, -1]]
    assert np.isinf(outlier_ref.split(keys)[0][:, 2:]).all() and outlier_ref.means(keys, 2).tolist() == [0.5, 0.5]
    # radius: more than nb_points within the radius, the point itself counted, the boundary inside
    assert outlier_ref.radius(pts, 1, 0.5).tolist() == [True, True, True, False, True, False]
    assert outlier_ref.radius(pts, 2, 1.0).tolist() == [True, True, True, False, False, False]
    assert outlier_ref.radius(pts, 0, 0.1).all() and not outlier_ref.radius(pts, 6, 1000.0).any()      # M <= nb_points: nothing


def test_restatement_agrees_with_kdtree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(12)
    target = rng.normal(0, 10, (4000, 3)).astype(np.float32)
    query = np.concatenate([rng.normal(0, 12, (1500, 3)), target[:50]]).astype(np.float32)
    for k in (1, 5, 20, 32):
        d2, idx = outlier_ref.nearest_k(target, query, k)
        dist, kidx = spatial.cKDTree(target.astype(np.float64)).query(query.astype(np.float64), k=k)
        dist, kidx = dist.reshape(len(query), k), kidx.reshape(len(query), k)
        assert np.allclose(np.sqrt(d2.astype(np.float64)), dist, rtol=1e-6, atol=1e-6)
        # continuous coordinates: the orders agree except where two float64 distances round to one float32 value
        differ = (idx != kidx).any(1)
        assert differ.mean() < 0.01
        assert np.array_equal(np.sort(idx[~differ], 1), np.sort(kidx[~differ], 1))
        assert np.all(idx[-50:, 0] == np.arange(50)) and np.all(d2[-50:, 0] == 0)
