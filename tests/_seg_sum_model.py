"""The segmented sum of dem-engine_amd/csrc/deme_seg_sum.h in numpy, addition by addition: the bits the device must give.

Stage one takes the sorted entries in blocks of 256.  A block scans its entries by run of equal keys in eight steps d = 1, 2, ...,
128 -- every entry whose key equals the key d entries back adds that entry's running sum to its own, all entries at once --, hands
its first and its last run to two partials and writes every run closed inside it straight to the output.  A block whose first
entry is uncounted writes two empty partials.  Stage two scans the partials the same way, 256 a round, and carries the run a round
ends with into the next one.  fp64 addition is commutative bit for bit, so only the shape of this tree matters, and that is what
the functions below repeat."""
import numpy as np

BLOCK = 256
NONE = 0xFFFFFFFF


def _scan(keys, v, n):
    """the inclusive scan by run of equal keys along axis 1 of keys (G, 256), v (G, 256, L), n (G, 256); in place"""
    d = 1
    while d < BLOCK:
        add = keys[:, d:] == keys[:, :-d]
        v[:, d:] = np.where(add[:, :, None], v[:, :-d] + v[:, d:], v[:, d:])  # (the right-hand side is evaluated before the store)
        n[:, d:] = np.where(add, n[:, :-d] + n[:, d:], n[:, d:])
        d <<= 1


def _blocks(keys, v, n):
    """rows padded to a multiple of 256 with key 0xFFFFFFFF and zeros, as (G, 256 ...)"""
    g = -(-len(keys) // BLOCK)
    pad = g * BLOCK - len(keys)
    keys = np.concatenate([keys, np.full(pad, NONE, np.uint32)]).reshape(g, BLOCK)
    v = np.concatenate([v, np.zeros((pad, v.shape[1]))]).reshape(g, BLOCK, -1)
    n = np.concatenate([n, np.zeros(pad, np.uint32)]).reshape(g, BLOCK)
    return keys, v, n


def seg_sum(keys, terms, n_keys):
    """sums (n_keys x lanes, float64) and counts (n_keys, uint32) of the rows of terms by ascending keys; keys >= n_keys: uncounted"""
    keys, terms = np.asarray(keys, np.uint32), np.asarray(terms, np.float64)
    lanes = terms.shape[1]
    sums, counts = np.zeros((n_keys, lanes)), np.zeros(n_keys, np.uint32)
    if not len(keys):  # nothing is launched
        return sums, counts
    counted = keys < n_keys
    k, v, n = _blocks(keys, np.where(counted[:, None], terms, 0.0), counted.astype(np.uint32))
    _scan(k, v, n)
    pk, pv, pn = [], [], []  # the partials, two a block
    for b in range(len(k)):
        if k[b, 0] >= n_keys:  # behind the counted entries
            pk += [NONE, NONE]
            pv += [np.zeros(lanes), np.zeros(lanes)]
            pn += [0, 0]
            continue
        first, last = k[b, 0], k[b, -1]
        run_end = np.append(k[b, 1:] != k[b, :-1], True)
        e = int(np.flatnonzero(run_end & (k[b] == first))[0])  # (the keys ascend: one run per key)
        pk += [first, last]
        pv += [v[b, e].copy(), v[b, -1].copy() if last != first else np.zeros(lanes)]
        pn += [n[b, e], n[b, -1] if last != first else 0]
        for t in np.flatnonzero(run_end & (k[b] != first) & (k[b] != last) & (k[b] < n_keys)):
            sums[k[b, t]], counts[k[b, t]] = v[b, t], n[b, t]
    pk, pv, pn = _blocks(np.array(pk, np.uint32), np.array(pv).reshape(-1, lanes), np.array(pn, np.uint32))
    _scan(pk, pv, pn)
    ck, cv, cn = NONE, np.zeros(lanes), np.uint32(0)  # the run the round before ended with
    for r in range(len(pk)):
        if pk[r, 0] >= n_keys:  # nothing counted from here on
            break
        same = pk[r] == ck
        pv[r][same] = cv + pv[r][same]
        pn[r][same] = cn + pn[r][same]
        if not same[0] and ck < n_keys:  # the carried run ended with its round
            sums[ck], counts[ck] = cv, cn
        for t in np.flatnonzero((pk[r, 1:] != pk[r, :-1]) & (pk[r, :-1] < n_keys)):
            sums[pk[r, t]], counts[pk[r, t]] = pv[r, t], pn[r, t]
        ck, cv, cn = pk[r, -1], pv[r, -1].copy(), pn[r, -1]
    if ck < n_keys:
        sums[ck], counts[ck] = cv, cn
    return sums, counts


def left_to_right(keys, terms, n_keys):
    """the same sums, added one entry after the other: what a thread walking its run alone would give"""
    terms = np.asarray(terms, np.float64)
    sums = np.zeros((n_keys, terms.shape[1]))
    for key, row in zip(np.asarray(keys).tolist(), terms):
        if key < n_keys:
            sums[key] += row
    return sums
