"""The ray path crosses the index build's one size threshold (a mesh of up to 200 000 faces is sorted on 21
code bits in two radix passes, a larger one on 30 bits in three) through the SAME function as sls_mesh_distance, but it is
the only caller whose index outlives the call — so the larger side is cast against here once, reused."""
import numpy as np
import pytest
import torch

import raycast_ref as R
from splat_loam_amd import evaluation

pytestmark = pytest.mark.gpu


def test_index_beyond_the_sort_threshold(device):
    n = 320                                                             # 2 n^2 = 204 800 faces > 200 000
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i * 0.05, j * 0.05, 0.25 * np.sin(i * 0.07) + 0.02 * j], -1).reshape(-1, 3).astype(np.float32)
    k = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([k, k + n + 1, k + 1], 1), np.stack([k + 1, k + n + 1, k + n + 2], 1)]).astype(np.int32)
    f = f[np.random.default_rng(5).permutation(len(f))]
    assert len(f) > 200_000
    o, d = R.rays_for(v, f, 192, seed=9)
    vt, ft = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    index = evaluation.mesh_ray_index(vt, ft)
    out = [evaluation.cast_rays(torch.from_numpy(o).to(device), torch.from_numpy(d).to(device), vt, ft, return_uv=True, index=index)
           for _ in range(2)]
    t, face, uv = (x.cpu().numpy() for x in out[0])
    ht, hface, huv = R.host().cast(v, f, o, d)
    assert (hface >= 0).sum() > 64
    assert np.array_equal(face, hface) and t.tobytes() == ht.tobytes() and uv.tobytes() == huv.tobytes()
    assert all(torch.equal(a, b) for a, b in zip(out[0], out[1]))
