"""The numpy statement of the cluster inspector (include/deme_hip.h: deme_inspect_clusters), written from the header's text.

Vertices: the owners of `vertex` (the caller builds the mask: own clump owners that are no ghost copies; in a slab also the ghost
copies).  Edges: the rows of class sphere-sphere (type 1) that deme_inspect_contacts counts -- (double)fx^2 + (double)fy^2 +
(double)fz^2 >= (double)thr^2 -- whose two owners are different vertices.  Label: the smallest owner id of the vertex's connected
component; 0xFFFFFFFF for an owner that is no vertex.  Table: one row per cluster with a counted owner (`counted`: a subset of the
vertices), labels ascending, with the number of counted owners, the sum of (double)m and the sum of (double)m * P, P the owner's
centre of mass in the world frame in float64 (tests/_fields64.py: positions)."""
import numpy as np

from tests._contact_sums64 import row_owners

NONE = 0xFFFFFFFF


def union_find(n, a, b):
    """an array union-find over ids 0 .. n-1 with the edges (a[k], b[k]): the smaller root wins; returns the root of every id"""
    parent = list(range(n))  # (a list: the loop below is Python's)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(np.asarray(a, np.int64).tolist(), np.asarray(b, np.int64).tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(x) for x in range(n)], np.int64).reshape(n)


def edges_of(whole, tables, vertex, thr):
    """(owner A, owner B) of every row that is an edge"""
    oA, oB = row_owners(whole, tables)
    f = whole["force"].astype(np.float64)
    thr = np.float64(np.float32(thr))
    counted = f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2] >= thr * thr
    vertex = np.asarray(vertex, bool)
    take = counted & (whole["type"] == 1) & vertex[oA] & vertex[oB] & (oA != oB)
    return oA[take], oB[take]


def clusters(X, owner_mass, vertex, whole, tables, thr, counted=None):
    """X: positions(); owner_mass: float32 per owner; vertex / counted: bool per owner (counted None: every vertex); whole / tables:
    the whole list with records and the owner tables.  Returns labels (uint32 per owner), summary (a dict as DemeClusterSummary),
    the table's columns label, size, mass, moment, and abs_moment (the sums of |term|)."""
    vertex = np.asarray(vertex, bool)
    counted = vertex if counted is None else np.asarray(counted, bool) & vertex
    n = len(vertex)
    a, b = edges_of(whole, tables, vertex, thr)
    root = union_find(n, a, b)
    labels = np.where(vertex, root, NONE).astype(np.uint32)
    o = np.flatnonzero(counted)
    size_of = np.bincount(root[o], minlength=n)
    rows = np.flatnonzero(size_of > 0)
    row_of = np.full(n, -1, np.int64)
    row_of[rows] = np.arange(len(rows))
    m = np.asarray(owner_mass, np.float32)[o].astype(np.float64)
    term = m[:, None] * np.asarray(X, np.float64)[o]
    mass, moment, abs_moment = np.zeros(len(rows)), np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    np.add.at(mass, row_of[root[o]], m)
    np.add.at(moment, row_of[root[o]], term)
    np.add.at(abs_moment, row_of[root[o]], np.abs(term))
    size = size_of[rows].astype(np.uint32)
    # (the summary of a single context, where every vertex is counted)
    largest = int(size.max()) if len(size) else 0
    summary = {"vertices": int(vertex.sum()), "edges": int(len(a)), "clusters": int(len(rows)), "singletons": int((size == 1).sum()),
               "largestSize": largest, "largestLabel": int(rows[size == largest].min()) if len(size) else NONE}
    return {"labels": labels, "summary": summary, "label": rows.astype(np.uint32), "size": size, "mass": mass, "moment": moment,
            "abs_moment": abs_moment}
