"""Hole filling (sls_mesh_boundary_loops, sls_mesh_fill_holes) restated in NumPy and pure Python — np.unique on the edge
keys, then a WALK along the next pointers (the device sorts by a union-find root instead), the float64 sums in the header's
order — and include/sls_fill_math.h compiled as plain C with a small sequential driver (`host()`), plus the case table and
the grid of settings the hole-filling tests share."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

import mesh_ref
from simplify_ref import segment_sum

ROOT = mesh_ref.ROOT
LONG = 64                       # SLS_FILL_LONG
CHUNK = 2048                    # FillChunks::kChunk of csrc/sls_fill.hip: the entries one workgroup scans or compacts
FILLED, SKIP_EDGES, SKIP_NONFINITE, SKIP_SIZE = 0, 1, 2, 3
STATUS = ("vertices", "triangles", "halfedges", "loops", "filled", "skipped_edges", "skipped_size", "skipped_nonfinite",
          "open_halfedges", "complex_vertices", "degenerate", "out_of_range", "needed_vertices", "needed_triangles", "overflow")
LOOP_WORDS = (2, 3, 8, 9, 10, 11)       # the words sls_mesh_boundary_loops fills; the others are 0, word 15 is 1


def room(V, T, capacity=0.25):
    """mesh_ops._fill_room: (cap_vertices, cap_triangles)"""
    cap_t = T + max(int(np.ceil(capacity * T)), 64)
    return V + (cap_t - T) // 4 + 1, cap_t


# ---- the restatement -------------------------------------------------------------------------------------------------
def live(V, T, counts):
    return (V, T) if counts is None else (min(int(counts[0]), V), min(int(counts[1]), T))


def loops(faces, V, counts=None):
    """(halfedges (B,2) int64, loop (B,) int64, cycles: per loop the half-edges in the order of the walk from its lowest one,
    dict of the words of LOOP_WORDS)"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    VL, TL = live(V, len(f), counts)
    f = f[:TL]
    deg = mesh_ref.degenerate(f, VL)
    ok = f[deg == 0]
    d = np.concatenate([ok[:, [0, 1]], ok[:, [1, 2]], ok[:, [2, 0]]])
    if len(d):
        _, inverse, owners = np.unique(np.sort(d, axis=1), axis=0, return_inverse=True, return_counts=True)
        d = d[owners[inverse.reshape(-1)] == 1]
        d = d[np.lexsort((d[:, 1], d[:, 0]))]
    B = len(d)
    out_n, in_n = np.bincount(d[:, 0], minlength=VL + 1), np.bincount(d[:, 1], minlength=VL + 1)
    simple = (out_n == 1) & (in_n == 1)
    leaving = {int(a): h for h, a in enumerate(d[:, 0])}            # read only where exactly one half-edge leaves a
    entering = {int(b): h for h, b in enumerate(d[:, 1])}
    loop, cycles, seen = np.full((B,), -1, np.int64), [], np.zeros((B,), bool)
    for h0 in range(B):
        if seen[h0]:
            continue
        chain, h = [h0], h0
        seen[h0] = True
        while simple[d[h, 1]]:                                      # forwards, until the chain closes or meets a complex vertex
            h = leaving[int(d[h, 1])]
            if seen[h]:
                break
            seen[h] = True
            chain.append(h)
        closed = simple[d[chain[-1], 1]] and leaving[int(d[chain[-1], 1])] == h0
        h = h0
        while not closed and simple[d[h, 0]]:                       # ... and backwards: the rest of an open component
            h = entering[int(d[h, 0])]
            if seen[h]:
                break
            seen[h] = True
            chain.append(h)
        if closed and simple[d[chain, 0]].all():
            loop[chain] = len(cycles)
            cycles.append(chain)
    touched = (out_n + in_n) > 0
    words = {2: B, 3: len(cycles), 8: int((loop < 0).sum()), 9: int((touched & ~simple).sum()), 10: int((deg != 0).sum()),
             11: int((deg == 2).sum())}
    return d, loop, cycles, words


def fill(vertices, faces, max_edges=64, max_size=0.0, cap_vertices=None, cap_triangles=None, counts=None, found=None):
    """(vertices' (V',3) float32, faces (cap_triangles,3) int64 with the rows beyond T' at -1, the 16 status words); `found`:
    what loops() gave for the same mesh"""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, T = len(v), len(f)
    VL, TL = live(V, T, counts)
    if cap_vertices is None:
        cap_vertices, cap_triangles = room(V, T)
    d, loop, cycles, words = found if found is not None else loops(f, V, counts)
    new_v, new_f, skipped = [], [], {SKIP_EDGES: 0, SKIP_NONFINITE: 0, SKIP_SIZE: 0}
    for cycle in cycles:
        L = len(cycle)
        ring = np.sort(d[cycle, 0])                                 # the loop's vertices in ascending index
        p = v[ring]
        with np.errstate(invalid="ignore", over="ignore"):
            if L > max_edges:
                verdict = SKIP_EDGES
            elif not np.isfinite(p).all():
                verdict = SKIP_NONFINITE
            else:
                ext = p.max(0).astype(np.float64) - p.min(0).astype(np.float64)
                verdict = SKIP_SIZE if max_size != 0 and not ((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2] <= max_size * max_size) else FILLED
        if verdict != FILLED:
            skipped[verdict] += 1
        elif L == 3:
            a, n1, n2 = d[cycle[0], 0], d[cycle[0], 1], d[cycle[1], 1]      # the walk starts at the lowest vertex
            new_f.append((a, n2, n1))
        else:
            c = VL + len(new_v)
            new_v.append((segment_sum(p.astype(np.float64)) / np.float64(L)).astype(np.float32))
            tails = d[cycle]
            new_f += [(b, a, c) for a, b in tails[np.argsort(tails[:, 0])]]
    need_v, need_t = VL + len(new_v), TL + len(new_f)
    over = int(need_v > cap_vertices or need_t > cap_triangles)
    filled = 0 if over else len(cycles) - sum(skipped.values())
    if over:
        new_v, new_f = [], []
    out_v = np.concatenate([v[:VL], np.asarray(new_v, dtype=np.float32).reshape(-1, 3)])
    out_f = np.full((cap_triangles, 3), -1, np.int64)
    out_f[:TL] = f[:TL]
    out_f[TL:TL + len(new_f)] = np.asarray(new_f, dtype=np.int64).reshape(-1, 3)
    status = [len(out_v), TL + len(new_f), words[2], words[3], filled, skipped[SKIP_EDGES], skipped[SKIP_SIZE], skipped[SKIP_NONFINITE],
              words[8], words[9], words[10], words[11], need_v, need_t, over, 1]
    return out_v, out_f, status


def loop_status(words):
    return [words.get(i, 0) for i in range(15)] + [1]


# ---- the header on the host ------------------------------------------------------------------------------------------
_DRIVER = r'''
#include <stdlib.h>
#include <string.h>
#include "sls_fill_math.h"

typedef struct { uint64_t ukey, dkey; int32_t a, b; } HalfEdge;

static int cmp_ukey(const void *pa, const void *pb)
{
    const uint64_t a = ((const HalfEdge *)pa)->ukey, b = ((const HalfEdge *)pb)->ukey;
    return a < b ? -1 : (a > b ? 1 : 0);
}
static int cmp_dkey(const void *pa, const void *pb)
{
    const uint64_t a = ((const HalfEdge *)pa)->dkey, b = ((const HalfEdge *)pb)->dkey;
    return a < b ? -1 : (a > b ? 1 : 0);
}
static uint32_t find(uint32_t *parent, uint32_t x)
{
    while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
    return x;
}

typedef struct {
    int32_t VL, TL;
    uint32_t B, loops;
    HalfEdge *he;                   /* B boundary half-edges in key order */
    uint32_t *out_n, *in_n, *leaving;       /* per vertex */
    int32_t *loop;                  /* per half-edge */
    uint32_t *start, *member;       /* loop k holds member[start[k] .. start[k + 1]): its half-edges in ascending tail */
    uint32_t words[16];
} Loops;

static void loops_free(Loops *s)
{
    free(s->he); free(s->out_n); free(s->in_n); free(s->leaving); free(s->loop); free(s->start); free(s->member);
}

/* rules 1 to 4 */
static void loops_build(int V, int T, const int32_t *faces, const uint32_t *in_counts, Loops *s)
{
    memset(s, 0, sizeof(*s));
    s->VL = in_counts ? sls_fill_live(in_counts[0], V) : V;
    s->TL = in_counts ? sls_fill_live(in_counts[1], T) : T;
    const int bits = sls_mesh_index_bits(V);
    HalfEdge *all = (HalfEdge *)malloc(sizeof(HalfEdge) * (3 * (size_t)s->TL + 1));
    size_t n = 0;
    for (int t = 0; t < s->TL; ++t) {
        const int32_t *f = faces + 3 * (size_t)t;
        const int deg = sls_mesh_degenerate(f, s->VL);
        if (deg) { s->words[SLS_FILL_W_DEGENERATE]++; if (deg == 2) s->words[SLS_FILL_W_RANGE]++; continue; }
        for (int e = 0; e < 3; ++e) {
            sls_fill_half_edge(f, e, &all[n].a, &all[n].b);
            all[n].ukey = sls_mesh_edge_key(f, e, bits);
            all[n].dkey = sls_fill_key(all[n].a, all[n].b, bits);
            ++n;
        }
    }
    qsort(all, n, sizeof(HalfEdge), cmp_ukey);
    s->he = (HalfEdge *)malloc(sizeof(HalfEdge) * (n + 1));
    for (size_t p = 0; p < n; ++p)
        if ((p == 0 || all[p - 1].ukey != all[p].ukey) && (p + 1 == n || all[p + 1].ukey != all[p].ukey)) s->he[s->B++] = all[p];
    free(all);
    qsort(s->he, s->B, sizeof(HalfEdge), cmp_dkey);
    const uint32_t B = s->B;
    s->out_n = (uint32_t *)calloc((size_t)V + 1, sizeof(uint32_t));
    s->in_n = (uint32_t *)calloc((size_t)V + 1, sizeof(uint32_t));
    s->leaving = (uint32_t *)calloc((size_t)V + 1, sizeof(uint32_t));
    for (uint32_t h = 0; h < B; ++h) { s->out_n[s->he[h].a]++; s->in_n[s->he[h].b]++; s->leaving[s->he[h].a] = h; }
    for (int v = 0; v < V; ++v)
        if ((s->out_n[v] | s->in_n[v]) && !sls_fill_simple(s->out_n[v], s->in_n[v])) s->words[SLS_FILL_W_COMPLEX]++;
    uint32_t *parent = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)B + 1));
    uint8_t *bad = (uint8_t *)calloc((size_t)B + 1, 1);
    for (uint32_t h = 0; h < B; ++h) parent[h] = h;
    for (uint32_t h = 0; h < B; ++h) {
        const int32_t b = s->he[h].b;
        if (!sls_fill_simple(s->out_n[b], s->in_n[b])) continue;
        uint32_t x = find(parent, h), y = find(parent, s->leaving[b]);
        if (x != y) { if (x < y) parent[y] = x; else parent[x] = y; }
    }
    for (uint32_t h = 0; h < B; ++h) {
        const int32_t a = s->he[h].a, b = s->he[h].b;
        if (!sls_fill_simple(s->out_n[a], s->in_n[a]) || !sls_fill_simple(s->out_n[b], s->in_n[b])) bad[find(parent, h)] = 1;
    }
    s->loop = (int32_t *)malloc(sizeof(int32_t) * ((size_t)B + 1));
    s->start = (uint32_t *)calloc((size_t)B + 2, sizeof(uint32_t));
    s->member = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)B + 1));
    for (uint32_t h = 0; h < B; ++h) {                              /* a root is its component's lowest half-edge: ascending roots = loop order */
        const uint32_t r = find(parent, h);
        if (bad[r]) { s->loop[h] = -1; s->words[SLS_FILL_W_OPEN]++; continue; }
        if (r == h) s->loop[h] = (int32_t)s->loops++;
        else s->loop[h] = s->loop[r];
        s->start[s->loop[h] + 1]++;
    }
    for (uint32_t k = 0; k < s->loops; ++k) s->start[k + 1] += s->start[k];
    uint32_t *at = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)s->loops + 1));
    memcpy(at, s->start, sizeof(uint32_t) * s->loops);
    for (uint32_t h = 0; h < B; ++h)
        if (s->loop[h] >= 0) s->member[at[s->loop[h]]++] = h;
    s->words[SLS_FILL_W_HALFEDGES] = B;
    s->words[SLS_FILL_W_LOOPS] = s->loops;
    s->words[SLS_FILL_W_WRITTEN] = 1u;
    free(parent); free(bad); free(at);
}

/* halfedges: room for 3 T pairs, loop: 3 T, loop_edges: T, status: 16 words */
void ref_loops(int V, int T, const int32_t *faces, const uint32_t *in_counts, int32_t *halfedges, int32_t *loop, int32_t *loop_edges,
               uint32_t *status)
{
    Loops s;
    loops_build(V, T, faces, in_counts, &s);
    for (uint32_t h = 0; h < s.B; ++h) { halfedges[2 * (size_t)h] = s.he[h].a; halfedges[2 * (size_t)h + 1] = s.he[h].b; loop[h] = s.loop[h]; }
    for (uint32_t k = 0; k < s.loops; ++k) loop_edges[k] = (int32_t)(s.start[k + 1] - s.start[k]);
    memcpy(status, s.words, sizeof(s.words));
    loops_free(&s);
}

/* "the order of every float64 sum", the box and the finite flag over the loop's vertices in ascending index */
static int loop_sums(const Loops *s, const float *xyz, uint32_t k, double acc[3], float lo[3], float hi[3])
{
    const uint32_t b = s->start[k], L = s->start[k + 1] - b;
    int finite = 1;
    for (int c = 0; c < 3; ++c) { acc[c] = 0.0; lo[c] = INFINITY; hi[c] = -INFINITY; }
    double part[64][3], next[64][3];
    memset(part, 0, sizeof(part));
    for (uint32_t j = 0; j < L; ++j) {
        const float *p = xyz + 3 * (size_t)s->he[s->member[b + j]].a;
        finite &= sls_fill_finite3(p);
        sls_fill_box(lo, hi, p);
        sls_fill_add(L <= SLS_FILL_LONG ? acc : part[j % 64], p);
    }
    if (L <= SLS_FILL_LONG) return finite;
    for (int off = 32; off > 0; off >>= 1) {
        for (int l = 0; l < 64; ++l) for (int c = 0; c < 3; ++c) next[l][c] = part[l][c] + part[l ^ off][c];
        memcpy(part, next, sizeof(part));
    }
    for (int c = 0; c < 3; ++c) acc[c] = part[0][c];
    return finite;
}

/* out_vertices: cap_vertices rows, out_faces: cap_triangles rows, status: 16 words */
void ref_fill(int V, const float *xyz, int T, const int32_t *faces, const uint32_t *in_counts, int max_edges, double max_size,
              int cap_vertices, float *out_vertices, int cap_triangles, int32_t *out_faces, uint32_t *status)
{
    Loops s;
    loops_build(V, T, faces, in_counts, &s);
    int *verdict = (int *)malloc(sizeof(int) * ((size_t)s.loops + 1));
    float *centre = (float *)malloc(sizeof(float) * 3 * ((size_t)s.loops + 1));
    uint64_t new_v = 0, new_t = 0;
    for (uint32_t k = 0; k < s.loops; ++k) {
        const uint32_t L = s.start[k + 1] - s.start[k];
        double acc[3];
        float lo[3], hi[3];
        int finite = 1;
        if (L <= (uint32_t)max_edges) finite = loop_sums(&s, xyz, k, acc, lo, hi);
        verdict[k] = sls_fill_verdict(L, finite, lo, hi, (uint32_t)max_edges, max_size);
        if (sls_fill_new_vertices(L, verdict[k])) sls_fill_centroid(acc, L, centre + 3 * (size_t)k);
        new_v += sls_fill_new_vertices(L, verdict[k]);
        new_t += sls_fill_new_triangles(L, verdict[k]);
        s.words[verdict[k] == SLS_FILL_FILLED ? SLS_FILL_W_FILLED : verdict[k] == SLS_FILL_SKIP_EDGES ? SLS_FILL_W_SKIP_EDGES
                : verdict[k] == SLS_FILL_SKIP_SIZE ? SLS_FILL_W_SKIP_SIZE : SLS_FILL_W_SKIP_NONFINITE]++;
    }
    const uint64_t need_v = (uint64_t)s.VL + new_v, need_t = (uint64_t)s.TL + new_t;
    const int over = need_v > (uint64_t)cap_vertices || need_t > (uint64_t)cap_triangles;
    memcpy(out_vertices, xyz, sizeof(float) * 3 * (size_t)s.VL);
    memcpy(out_faces, faces, sizeof(int32_t) * 3 * (size_t)s.TL);
    size_t nv = (size_t)s.VL, nt = (size_t)s.TL;
    for (uint32_t k = 0; k < s.loops && !over; ++k) {
        const uint32_t b = s.start[k], L = s.start[k + 1] - b;
        if (verdict[k] != SLS_FILL_FILLED) continue;
        if (L == 3u) {
            const HalfEdge *h0 = &s.he[s.member[b]];                /* leaves the lowest vertex */
            out_faces[3 * nt] = h0->a; out_faces[3 * nt + 1] = s.he[s.leaving[h0->b]].b; out_faces[3 * nt + 2] = h0->b;
            ++nt;
            continue;
        }
        memcpy(out_vertices + 3 * nv, centre + 3 * (size_t)k, 12);
        for (uint32_t j = 0; j < L; ++j) {
            const HalfEdge *h = &s.he[s.member[b + j]];
            out_faces[3 * nt] = h->b; out_faces[3 * nt + 1] = h->a; out_faces[3 * nt + 2] = (int32_t)nv;
            ++nt;
        }
        ++nv;
    }
    for (size_t i = 3 * nt; i < 3 * (size_t)cap_triangles; ++i) out_faces[i] = -1;
    if (over) s.words[SLS_FILL_W_FILLED] = 0;
    s.words[SLS_FILL_W_VERTICES] = (uint32_t)nv;
    s.words[SLS_FILL_W_TRIANGLES] = (uint32_t)nt;
    s.words[SLS_FILL_W_NEED_VERTICES] = (uint32_t)need_v;
    s.words[SLS_FILL_W_NEED_TRIANGLES] = (uint32_t)need_t;
    s.words[SLS_FILL_W_OVERFLOW] = (uint32_t)over;
    memcpy(status, s.words, sizeof(s.words));
    free(verdict); free(centre);
    loops_free(&s);
}
'''


def _counts(counts):
    return None if counts is None else np.asarray(counts, dtype=np.uint32)


class Host:
    """include/sls_fill_math.h compiled as plain C and called through ctypes."""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_loops.restype = None
        lib.ref_loops.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6
        lib.ref_fill.restype = None
        lib.ref_fill.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p]

    def loops(self, faces, V, counts=None):
        """(halfedges (B,2) int32, loop (B,) int32, loop_edges (L,) int32, status: 16 words); V == 0 or T == 0 as the C entry"""
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        T, c = len(f), _counts(counts)
        if V == 0 or T == 0:
            return np.zeros((0, 2), np.int32), np.zeros((0,), np.int32), np.zeros((0,), np.int32), empty_status(V, T, counts, False)
        he, loop = np.zeros((3 * T, 2), np.int32), np.zeros((3 * T,), np.int32)
        edges, status = np.zeros((T,), np.int32), np.zeros((16,), np.uint32)
        self.lib.ref_loops(V, T, f.ctypes.data, None if c is None else c.ctypes.data, he.ctypes.data, loop.ctypes.data, edges.ctypes.data,
                           status.ctypes.data)
        B, L = int(status[2]), int(status[3])
        return he[:B], loop[:B], edges[:L], [int(x) for x in status]

    def fill(self, vertices, faces, max_edges=64, max_size=0.0, cap_vertices=None, cap_triangles=None, counts=None):
        """(vertices' (V',3) float32, faces (cap_triangles,3) int32 with the rows beyond T' at -1, status: 16 words)"""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
        V, T, c = len(v), len(f), _counts(counts)
        if cap_vertices is None:
            cap_vertices, cap_triangles = room(V, T)
        out_v, out_f = np.zeros((cap_vertices + 1, 3), np.float32), np.zeros((cap_triangles + 1, 3), np.int32)
        status = np.zeros((16,), np.uint32)
        if V == 0 or T == 0:
            VL, TL = live(V, T, counts)
            out_v[:VL], out_f[:TL], out_f[TL:] = v[:VL], f[:TL], -1
            return out_v[:VL], out_f[:cap_triangles], empty_status(V, T, counts, True)
        self.lib.ref_fill(V, v.ctypes.data, T, f.ctypes.data, None if c is None else c.ctypes.data, int(max_edges), float(max_size),
                          int(cap_vertices), out_v.ctypes.data, int(cap_triangles), out_f.ctypes.data, status.ctypes.data)
        return out_v[:int(status[0])], out_f[:cap_triangles], [int(x) for x in status]


def empty_status(V, T, counts, fills):
    """the words of a call without a vertex or without a triangle (sls_abi.h): no half-edge; V == 0: every live row is out of range"""
    VL, TL = live(V, T, counts)
    w = [0] * 15 + [1]
    w[10] = w[11] = TL
    if fills:
        w[0] = w[12] = VL
        w[1] = w[13] = TL
    return w


_KEEP = []


@functools.lru_cache(maxsize=None)
def host():
    d = tempfile.TemporaryDirectory(prefix="fill_ref_")
    _KEEP.append(d)
    src = os.path.join(d.name, "fill_host.c")
    with open(src, "w") as f:
        f.write(_DRIVER)
    so = os.path.join(d.name, "libfill_host.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), src,
                           "-o", so, "-lm"])
    return Host(C.CDLL(so))


# ---- the case table --------------------------------------------------------------------------------------------------
def _f32(points):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3)


def _i32(faces):
    return np.asarray(faces, dtype=np.int32).reshape(-1, 3)


TET_V = [(0, 0, 0), (1, 0.1, 0), (0.2, 1, 0.1), (0.3, 0.2, 1)]
TET_F = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)]
CUBE_V = [(x, y, z) for z in (0, 1) for y in (0, 1) for x in (0, 1)]
CUBE_F = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]


def sheet(n, holes=(), seed=3):
    """an n x n sheet of vertices 0.25 apart with seeded z-noise, two triangles per square (all of one orientation); `holes`:
    the squares (x, y) left out"""
    rng = np.random.default_rng(seed + n)
    xy = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="xy"), 2).reshape(-1, 2) * 0.25
    v = np.concatenate([xy, 0.3 + 0.02 * rng.uniform(-1.0, 1.0, (n * n, 1))], 1)
    holes = set(holes)
    quads = [(n * y + x, n * y + x + 1, n * y + x + n + 1, n * y + x + n) for y in range(n - 1) for x in range(n - 1) if (x, y) not in holes]
    return _f32(v), _i32([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


MANY_CELLS = 79


def many_loops():
    """every second square of every second row of a sheet of 159 x 159 squares left out: MANY_CELLS^2 = 6241 loops of 4
    half-edges and the outer rim of 636, B = 25 600 — the loops and B are each more than three times FillChunks::kChunk = 2048, the
    entries one workgroup of every scan and compaction of sls_fill.hip handles (6241 > 3 x 2048 = 6144, B = 12.5 x 2048);
    25 600 vertices, 38 080 triangles"""
    n = 2 * MANY_CELLS + 2
    return sheet(n, [(2 * i + 1, 2 * j + 1) for i in range(MANY_CELLS) for j in range(MANY_CELLS)])


SPHERE_CUTS = (("z", 2, 0.9, 1), ("y", 1, 0.6, 1), ("z", 2, -0.5, -1), ("x", 0, -0.8, -1))


@functools.lru_cache(maxsize=None)
def welded_sphere():
    v, index = mesh_ref.weld(mesh_ref.sphere_soup())
    return v, index.reshape(-1, 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def sphere_caps():
    """the welded marching-tetrahedra sphere (3578 vertices, 7152 triangles) without the triangles whose three vertices all lie
    beyond one of SPHERE_CUTS (world coordinates), without the one-ring of the first vertex of valence 8 that touches no rim,
    and without the first triangle that touches neither: loops of 65, 64, 89 and 35 half-edges (the 64-item switch from both
    sides), one of 8 and one of 3.  (vertices, faces), read-only"""
    v, f = welded_sphere()
    keep = np.ones((len(f),), bool)
    for _, axis, bound, sign in SPHERE_CUTS:
        c = v[:, axis][f]
        keep &= ~((c > bound).all(1) if sign > 0 else (c < bound).all(1))
    rim = np.zeros((len(v),), bool)
    rim[f[~keep].reshape(-1)] = True                                # every vertex of a removed triangle
    valence = np.bincount(f.reshape(-1), minlength=len(v))
    near = np.zeros((len(v),), bool)                                # the vertices with a rim vertex in their one-ring
    near[f[rim[f].any(1)].reshape(-1)] = True
    hub = int(np.nonzero((valence == 8) & ~near)[0][0])
    ring = (f == hub).any(1)
    taken = rim.copy()
    taken[f[ring].reshape(-1)] = True
    near[f[taken[f].any(1)].reshape(-1)] = True
    single = int(np.nonzero(keep & ~ring & ~near[f].any(1))[0][0])
    keep &= ~ring
    keep[single] = False
    g = np.ascontiguousarray(f[keep])
    g.setflags(write=False)
    return v, g


SPHERE_LOOPS = (65, 64, 89, 35, 8, 3)
SIZE_SPLIT = 0.5                # between the diagonals of the sphere's two small loops and of its four caps


def at_capacity():
    """a sheet with two holes at capacity: rows of -1 and degenerate rows inside the live range, live counts below V and T with
    garbage beyond them (NaN vertices, faces that point past V_live and would close a hole), unreferenced vertex rows in the
    middle.  (vertices, faces, counts)"""
    v, f = sheet(7, [(1, 1), (4, 3)])
    v = np.concatenate([v[:20], _f32([(9, 9, 9), (-0.0, -0.0, -0.0)]), v[20:]])          # two unreferenced rows: indices 20 and 21
    f = np.where(f >= 20, f + 2, f)
    VL = len(v)
    f = np.concatenate([f[:10], _i32([(-1, -1, -1), (3, 3, 4), (0, VL, 1)]), f[10:], _i32([(-1, -1, -1)])])
    TL = len(f)
    nan = np.float32(np.nan)
    v = np.concatenate([v, _f32([(nan, nan, nan), (nan, 0, 0), (1, 1, 1)])])
    a = 7 + 1 + 2                                                   # the corners of the hole (1, 1): vertices 8, 9, 16, 15 of the 7 x 7 sheet
    f = np.concatenate([f, _i32([(a - 2, a - 1, VL), (a - 2, 16, 15), (VL, VL + 1, VL + 2), (-1, -1, -1)])])
    return v, f, (VL, TL)


def rings(sizes=(64, 65, 100), seed=5):
    """annuli between two rings of n vertices each, one after the other: two loops of n half-edges per annulus.  In every
    ring and coordinate a seeded half of the vertices hold values around 2^30 that cancel in pairs, the others values around
    1: a float64 sum of them loses bits of the small ones that depend on its order, so the order of a sum of more than 64
    shows in the float32 centroid — the lattice coordinates of the sphere add exactly in any order"""
    rng = np.random.default_rng(seed)
    vs, fs, base = [], [], 0
    for n in sizes:
        v = rng.uniform(-1.0, 1.0, (2 * n, 3)).astype(np.float32)
        for ring in (0, n):
            for axis in range(3):
                pick = ring + rng.permutation(n)[:n // 4 * 2]
                big = (rng.uniform(1.0, 2.0, len(pick) // 2) * 2.0 ** 30).astype(np.float32)
                v[pick[0::2], axis], v[pick[1::2], axis] = big, -big
        vs.append(v)
        i = np.arange(n)
        j = (i + 1) % n
        fs.append(np.concatenate([np.stack([i, j, n + i], 1), np.stack([j, n + j, n + i], 1)]) + base)
        base += 2 * n
    return _f32(np.concatenate(vs)), _i32(np.concatenate(fs))


STRIPS = (682, 683, 1365, 1366)     # 3 T = 2046, 2049, 4095, 4098 sorted pairs: either side of one and of two chunks of CHUNK entries


def strip(T, seed=13):
    """an open strip of T triangles of one orientation over T + 2 vertices on two rows with seeded noise: no hole, the rim
    one loop of T + 2 half-edges (longer than every max_edges of settings(): found, never filled)"""
    rng = np.random.default_rng(seed + T)
    i = np.arange(T + 2)
    v = np.stack([0.125 * i, 0.25 * (i % 2), 0.3 + 0.02 * rng.uniform(-1.0, 1.0, T + 2)], 1)
    t = np.arange(T)
    return _f32(v), _i32(np.stack([np.where(t % 2 == 0, t, t + 1), np.where(t % 2 == 0, t + 1, t), t + 2], 1))


def cases():
    """name -> (vertices (V,3) float32, faces (T,3) int32, counts or None)"""
    nan = np.float32(np.nan)
    out = {}
    out["tet_open"] = (_f32(TET_V), _i32(TET_F[:3]), None)                                              # L = 3: one triangle, no vertex
    out["cube_open"] = (_f32(CUBE_V), _i32(CUBE_F[2:]), None)                                           # L = 4: one centre
    out["triangle"] = (_f32(TET_V[:3]), _i32([(0, 1, 2)]), None)                                        # its own rim: filled by (0, 2, 1)
    out["sphere_caps"] = sphere_caps() + (None,)
    out["pinch"] = sheet(6, [(1, 1), (2, 2)]) + (None,)                                                 # two holes that share vertex (2, 2)
    v, f = sheet(6, [(2, 2)])
    g = f.copy()
    g[np.nonzero((f == 2 * 6 + 2).any(1) & (f == 2 * 6 + 3).any(1))[0][0]] = g[np.nonzero((f == 2 * 6 + 2).any(1) & (f == 2 * 6 + 3).any(1))[0][0]][::-1]
    out["flipped"] = (v, g, None)                                                                       # a rim triangle the other way round
    # a third owner on the edge from the rim's corner 14 to its neighbour 8: 14 and 8 are complex, the rim stays open
    out["fin"] = (np.concatenate([v, _f32([(0.6, 0.3, 1.0)])]), np.concatenate([f, _i32([(8, 14, 36)])]), None)
    out["at_capacity"] = at_capacity()
    v, f = sheet(8, [(1, 1), (4, 2), (2, 5)])
    v = v.copy()
    v[8 * 2 + 4, 1] = nan                                                                               # a corner of the hole (4, 2)
    out["nan_rim"] = (v, f, None)
    out["rings"] = rings() + (None,)                                                                    # loops of 64, 65 and 100, twice each
    out["many_loops"] = many_loops() + (None,)
    for T in STRIPS:                                                                                    # the edges of the scans' chunks
        out[f"strip_{T}"] = strip(T) + (None,)
    out["closed"] = (_f32(TET_V), _i32(TET_F), None)
    out["no_faces"] = (_f32(TET_V), _i32([]), None)
    out["no_vertices"] = (_f32([]), _i32([]), None)
    return out


def settings():
    """(max_edges, max_size): 3 (triangles alone), 64 (the default: the switch to the butterfly is not taken), 128 (it is), each
    without a size limit and with one that splits the sphere's loops"""
    return [(e, s) for e in (3, 64, 128) for s in (0.0, SIZE_SPLIT)]
