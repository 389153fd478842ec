"""The pseudo-normal build at a size where its sorts take their larger paths: the wavy 320 x 320 grid of
tests/test_raycast_scale.py, 204 800 shuffled faces — past the index build's sort threshold of 200 000 faces — and 614 400
corners, which is more than one workgroup of chunk totals in the sorter's shared scan.  Tables, status and results equal
the header on the host bit for bit, and two runs are equal."""
import numpy as np
import pytest
import torch

import meshdist_ref
import signdist_ref as R
from splat_loam_amd import evaluation

pytestmark = pytest.mark.gpu


def test_tables_and_sign_beyond_the_sort_thresholds(device):
    v, f = R.wavy_grid()
    assert len(f) == 204800 > 200_000
    q = meshdist_ref.queries_for(v, f, 192, seed=9)
    hfn, hen, hvn, hstatus = tables = R.host().tables(v, f)
    hsd, hface, hclosest, hfeature = R.host().query(v, f, tables, q)
    assert hstatus.tolist() == [0, 0, 0, 0, 4 * 320, 0, 0, 1]            # an open, manifold, consistently oriented sheet
    vt, ft, qt = torch.from_numpy(np.array(v)).to(device), torch.from_numpy(np.array(f)).to(device), torch.from_numpy(q).to(device)
    runs = []
    for _ in range(2):
        pn = evaluation.mesh_pseudonormals(vt, ft)
        out = evaluation.signed_distance(qt, vt, ft, return_face=True, return_closest=True, return_feature=True, pseudonormals=pn)
        runs.append((pn.status, pn.face_normals, pn.edge_normals, pn.vertex_normals) + tuple(out))
    status, fn, en, vn, sd, face, closest, feature = (x.cpu().numpy() for x in runs[0])
    assert status.astype(np.uint32).tolist() == hstatus.tolist()
    assert fn.tobytes() == hfn.tobytes() and en.tobytes() == hen.tobytes() and vn.tobytes() == hvn.tobytes()
    assert np.array_equal(face, hface) and np.array_equal(feature, hfeature)
    assert sd.tobytes() == hsd.tobytes() and closest.tobytes() == hclosest.tobytes()
    assert (sd < 0).sum() > 16 and (sd > 0).sum() > 16
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
