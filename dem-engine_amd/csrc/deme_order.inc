// deme_order.inc -- the engine's own spatial numbering of clumps and spheres (included by deme_hip.hip).
//
// The reference numbers owners in load order (DEM/dT.cpp:700-800: clumps are flattened as the script loaded them) and every id the
// user sees -- trackers, contact pair files, wildcard arrays -- is in that numbering.  The owner-tile force pass (deme_tile.h)
// wants 128 CONSECUTIVE owners to be a compact cluster of the bed.  So the engine keeps its own order: at deme_upload_scene the
// clumps are cut into box-shaped tiles of 128 by recursive bisection (order_bisect), the spheres follow their clumps, and two maps -- engine slot -> caller id (o2e, s2e) and back (e2o, e2s) -- translate at the C-ABI:
// state up- and downloads, margins, contact lists (ids AND list order: a downloaded list is in the caller's canonical order, by
// sphere A, class, B of the caller's ids), contact wildcards and records, persistent contacts, sphere geometry, per-owner
// inspection values, added accelerations, exchange lists.  Inside, which sphere of a pair is A follows
// the CALLER's ids too (deme_kernels.h: a_before_b), so lists, contact points and histories are exactly those of the caller's
// numbering; only the order in which an owner's contributions are summed differs -- which is why the EXACT arithmetic mode, whose
// contract is bit-identity with the oracle, keeps the caller's order, as do slabs with ghosts (their order is the decomposition's,
// bench.py builds it along the curve already).  A run-time compiled force model sees the caller's ids (AOwner, AGeo ... are
// translated where the vocabulary is filled) and its owner / sphere wildcard arrays stay in the caller's order.
//
// DEME_REORDER=0 switches the engine-side order off (A/B runs; the row-major 1e6 bed of tests/test_full_size.py).

namespace {

inline uint64_t morton_spread21(uint64_t v) {  // 21 bits -> every third bit
    v &= 0x1FFFFFull;
    v = (v | (v << 32)) & 0x1F00000000FFFFull;
    v = (v | (v << 16)) & 0x1F0000FF0000FFull;
    v = (v | (v << 8)) & 0x100F00F00F00F00Full;
    v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

// position of a clump in sub-voxel units per axis (the codec's integers: exact, no rounding to argue about)
inline void order_units_of(const DemeParams& hp, uint64_t voxelID, uint16_t lx, uint16_t ly, uint16_t lz, uint64_t u[3]) {
    const uint64_t vx = voxelID & ((1ull << hp.nvXp2) - 1), vy = (voxelID >> hp.nvXp2) & ((1ull << hp.nvYp2) - 1),
                   vz = voxelID >> (hp.nvXp2 + hp.nvYp2);
    u[0] = (vx << 16) | lx, u[1] = (vy << 16) | ly, u[2] = (vz << 16) | lz;
}

// mean surface of the bounding box of a tile of DEME_TILE_NB consecutive clumps, in squares of one bin edge: how compact an order
// is -- the foreign owners a tile has to stage live across that surface (a row of 128 clumps has the volume of a 5 x 5 x 5 cluster,
// not its surface)
double order_tile_spread(const DemeParams& hp, const std::vector<uint64_t>& units /* 3 per clump */, const uint32_t* ord, size_t nClumps) {
    const double cell = hp.binSize / hp.l;
    double sum = 0;
    size_t nT = 0;
    for (size_t t0 = 0; t0 < nClumps; t0 += DEME_TILE_NB, nT++) {
        uint64_t lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
        for (size_t i = t0; i < std::min(nClumps, t0 + DEME_TILE_NB); i++) {
            const size_t q = ord ? ord[i] : i;
            for (int k = 0; k < 3; k++)
                lo[k] = std::min(lo[k], units[3 * q + k]), hi[k] = std::max(hi[k], units[3 * q + k]);
        }
        const double ex = (double)(hi[0] - lo[0]) / cell + 1.0, ey = (double)(hi[1] - lo[1]) / cell + 1.0, ez = (double)(hi[2] - lo[2]) / cell + 1.0;
        sum += ex * ey + ey * ez + ez * ex;
    }
    return nT ? sum / (double)nT : 0.0;
}

// The engine's order of n clumps: recursive bisection into tiles.  A set of T tiles' worth of clumps is cut across the longest side
// of its bounding box into the first floor(T / 2) * DEME_TILE_NB clumps along that axis and the rest, down to single tiles: every
// tile is a box-shaped cluster of exactly DEME_TILE_NB clumps whatever the packing (a Z-order curve over cells gives tiles that
// are unions of partial octants -- measured on the 1e6 bed: largest halo 177 against 144 for an exact octant order, which costs the
// tile kernel a workgroup per CU --, bisection gives 130-140), and consecutive tiles are neighbours in space.  Inside a tile the
// clumps follow a Z-order curve.  O(n log(n / 128)) on the host, at upload time.
void order_bisect(const std::vector<uint64_t>& units, std::vector<uint32_t>& ord, unsigned fineShift) {
    const size_t n = ord.size();
    struct Job {
        size_t b, e;
    };
    std::vector<Job> stack{{0, n}};
    while (!stack.empty()) {
        const Job j = stack.back();
        stack.pop_back();
        const size_t m = j.e - j.b, tiles = (m + DEME_TILE_NB - 1) / DEME_TILE_NB;
        if (tiles <= 1) {
            // inside a tile: along a Z-order curve over cells of an eighth of a bin edge (ties by the caller's id) -- the bin sweep and
            // the sphere kernels gather 32-byte records of spheres that are neighbours in space: they should be neighbours in
            // memory down to the cache line (measured: the sweep's fetches grew from 216 to 263 MB with the caller's order inside)
            std::sort(ord.begin() + j.b, ord.begin() + j.e, [&](uint32_t a, uint32_t b) {
                const uint64_t* ua = &units[3 * (size_t)a];
                const uint64_t* ub = &units[3 * (size_t)b];
                const uint64_t ka = morton_spread21(ua[0] >> fineShift) | (morton_spread21(ua[1] >> fineShift) << 1) | (morton_spread21(ua[2] >> fineShift) << 2);
                const uint64_t kb = morton_spread21(ub[0] >> fineShift) | (morton_spread21(ub[1] >> fineShift) << 1) | (morton_spread21(ub[2] >> fineShift) << 2);
                return ka != kb ? ka < kb : a < b;
            });
            continue;
        }
        uint64_t lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0};
        for (size_t i = j.b; i < j.e; i++)
            for (int k = 0; k < 3; k++)
                lo[k] = std::min(lo[k], units[3 * (size_t)ord[i] + k]), hi[k] = std::max(hi[k], units[3 * (size_t)ord[i] + k]);
        int ax = 0;
        for (int k = 1; k < 3; k++)
            if (hi[k] - lo[k] > hi[ax] - lo[ax])
                ax = k;
        const size_t left = (tiles / 2) * DEME_TILE_NB;
        std::nth_element(ord.begin() + j.b, ord.begin() + j.b + left, ord.begin() + j.e, [&](uint32_t a, uint32_t b) {
            const uint64_t ua = units[3 * (size_t)a + ax], ub = units[3 * (size_t)b + ax];
            return ua != ub ? ua < ub : a < b;  // (ties by id: the order is a function of the scene, not of the library's sort)
        });
        stack.push_back({j.b + left, j.e});
        stack.push_back({j.b, j.b + left});
    }
}

// order of nC clumps given their encoded positions; spread[0] / [1]: tile surface in the given order / in the computed one
void order_compute(const DemeParams& hp, size_t nC, const uint64_t* voxelID, const uint16_t* lx, const uint16_t* ly, const uint16_t* lz,
                   std::vector<uint32_t>& ord, double spread[2]) {
    std::vector<uint64_t> units(3 * nC);
    for (size_t i = 0; i < nC; i++)
        order_units_of(hp, voxelID[i], lx[i], ly[i], lz[i], &units[3 * i]);
    ord.resize(nC);
    for (size_t i = 0; i < nC; i++)
        ord[i] = (uint32_t)i;
    unsigned fineShift = 0;  // cells of (at least) an eighth of a bin edge, as a shift of the position units
    while (fineShift < 60 && (double)(1ull << (fineShift + 1)) <= 0.125 * hp.binSize / hp.l)
        fineShift++;
    order_bisect(units, ord, fineShift);
    spread[0] = order_tile_spread(hp, units, nullptr, nC), spread[1] = order_tile_spread(hp, units, ord.data(), nC);
}

// Decide the engine's order for a scene about to be uploaded.  Fills the four host maps (identity beyond the clumps) and returns
// true if the order differs from the caller's.
bool order_decide(deme_ctx* c, const DemeScene* s) {
    const size_t nO = s->nOwners, nC = s->nOwnerClumps, nS = s->nSpheres;
    c->hO2E.clear(), c->hE2O.clear(), c->hS2E.clear(), c->hE2S.clear();
    c->orderSpread[0] = c->orderSpread[1] = 0;
    c->orderEligible = c->orderStructOK = false;
    static const int envOn = getenv("DEME_REORDER") ? atoi(getenv("DEME_REORDER")) : 1;
    if (!envOn || !c->reorderEnable || !c->haveParams || s->ownerGhost || nC <= 2 * (size_t)DEME_TILE_NB || !(c->hp.binSize > 0) ||
        !(c->hp.l > 0))
        return false;
    // (spheres are clump-major: deme_upload_scene checked it -- the sphere order follows from the clump order)
    c->orderStructOK = true;  // what does not depend on the arithmetic mode (deme_set_arith_mode re-derives orderEligible from it)
    if (c->arith != DEME_ARITH_FAST)  // the exact mode sums an owner's contributions in the CALLER's order: bit-identity with the oracle
        return false;
    c->orderEligible = true;
    std::vector<uint32_t> ord;
    order_compute(c->hp, nC, s->voxelID, s->locX, s->locY, s->locZ, ord, c->orderSpread);
    // an order that is already compact stays as it is (a bed the caller numbered along a curve: no translation at the ABI)
    if (c->orderSpread[0] <= 1.15 * c->orderSpread[1])
        return false;
    c->hO2E.resize(nO), c->hE2O.resize(nO), c->hS2E.resize(nS), c->hE2S.resize(nS);
    for (size_t i = 0; i < nC; i++)
        c->hO2E[i] = ord[i], c->hE2O[ord[i]] = (uint32_t)i;
    for (size_t i = nC; i < nO; i++)
        c->hO2E[i] = c->hE2O[i] = (uint32_t)i;
    // spheres: first sphere of every clump in the caller's list, then the clumps in engine order
    std::vector<uint32_t> first(nC + 1, 0);
    for (size_t i = 0; i < nS; i++)
        if (s->ownerClumpBody[i] < nC)
            first[s->ownerClumpBody[i] + 1]++;
    for (size_t i = 0; i < nC; i++)
        first[i + 1] += first[i];
    size_t w = 0;
    for (size_t i = 0; i < nC; i++)
        for (uint32_t e = first[ord[i]]; e < first[ord[i] + 1]; e++, w++)
            c->hS2E[w] = e, c->hE2S[e] = (uint32_t)w;
    for (size_t i = first[nC]; i < nS; i++, w++)  // (spheres of owners beyond the clumps: none in a well-formed scene)
        c->hS2E[w] = (uint32_t)i, c->hE2S[i] = (uint32_t)w;
    return true;
}

// device copies of the slot -> caller id maps, DevParams
int order_upload_maps(deme_ctx* c) {
    c->dp.s2e = c->dp.o2e = nullptr;
    if (!c->permuted)
        return DEME_OK;
    if (int rc = upload(c, c->dO2E, c->hO2E.data(), c->hO2E.size()))
        return rc;
    if (int rc = upload(c, c->dS2E, c->hS2E.data(), c->hS2E.size()))
        return rc;
    HIPCK(hipStreamSynchronize(c->stream));
    c->dp.o2e = c->dO2E.as<uint32_t>(), c->dp.s2e = c->dS2E.as<uint32_t>();
    return DEME_OK;
}

inline uint32_t order_owner_in(const deme_ctx* c, uint32_t e) { return c->permuted ? c->hE2O[e] : e; }
inline uint32_t order_sphere_in(const deme_ctx* c, uint32_t e) { return c->permuted ? c->hE2S[e] : e; }
inline uint32_t order_sphere_out(const deme_ctx* c, uint32_t i) { return c->permuted ? c->hS2E[i] : i; }

// a key of the engine's list in the caller's ids (sphere A always; B a sphere only for sphere-sphere pairs)
inline uint64_t order_key_out(const deme_ctx* c, uint64_t k) {
    if (!c->permuted)
        return k;
    const uint32_t cls = key_class(k);
    return make_key(cls, c->hS2E[key_a(k)], cls == DEME_KEY_CLASS_SS ? c->hS2E[key_b(k)] : key_b(k));
}
inline uint64_t order_key_in(const deme_ctx* c, uint64_t k) {
    if (!c->permuted)
        return k;
    const uint32_t cls = key_class(k);
    return make_key(cls, c->hE2S[key_a(k)], cls == DEME_KEY_CLASS_SS ? c->hE2S[key_b(k)] : key_b(k));
}

// The caller's view of a sorted key list held in the engine's numbering: the keys in the caller's ids, in the caller's canonical
// order, and for every row the index it has in the engine's list.
int order_view_of(deme_ctx* c, const uint64_t* dKeys, size_t n, std::vector<uint64_t>& keysOut, std::vector<uint32_t>& perm) {
    keysOut.resize(n), perm.resize(n);
    std::vector<uint64_t> k(n);
    if (n)
        HIPCK(hipMemcpyAsync(k.data(), dKeys, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
        k[i] = order_key_out(c, k[i]), perm[i] = (uint32_t)i;
    if (c->permuted)
        std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
    for (size_t i = 0; i < n; i++)
        keysOut[i] = k[perm[i]];
    return DEME_OK;
}

// ... of the CURRENT list, cached until the list changes (deme_ctx::listSerial)
int order_current_view(deme_ctx* c) {
    if (c->viewSerial == c->listSerial && c->viewPerm.size() == c->nContacts)
        return DEME_OK;
    if (int rc = order_view_of(c, c->keysSorted[c->keysCur].as<uint64_t>(), c->nContacts, c->viewKeys, c->viewPerm))
        return rc;
    c->viewSerial = c->listSerial;
    return DEME_OK;
}

// Has the bed drifted away from the order it was given?  Called by every detection that built tiles, with their counters: the
// mean halo of the fitting tiles and the tiles that do not fit, against what they were at the first detection after the last
// ordering.  Sets orderRenewDue (order_renew at the next detection).
void order_watch_drift(deme_ctx* c, const RangeCounters& hr) {
    if (!c->orderEligible)
        return;
    const uint32_t nTiles = (c->nOwners + DEME_TILE_NB - 1) / DEME_TILE_NB;
    const uint32_t fit = std::max(1u, nTiles - std::min(nTiles, hr.nBig));
    const uint32_t mean16 = (uint32_t)(16ull * hr.tileHaloSum / fit);
    if (!c->orderBaseHalo) {
        c->orderBaseHalo = std::max(mean16, 16u);
        c->orderDetAt = c->nDetections;
    } else if (c->nDetections - c->orderDetAt >= 20 && nTiles > 4 &&
               (hr.nBig > std::max(4u, nTiles / 64u) || mean16 > c->orderBaseHalo + c->orderBaseHalo / 2)) {
        c->orderRenewDue = true;
    }
}

}  // namespace

// Renew the engine's order of a RUNNING simulation (a mixer, a flowing bed: the clumps drift away from the tiles they were put in,
// the tiles' halos grow, tiles stop fitting -- order_watch_drift watches both and sets orderRenewDue; deme_renew_order forces it).
// Called at the start of a detection, on a synchronised context: the owners' positions come to the host, the order is computed as
// at upload (order_compute), and everything that is kept in engine slots follows -- owner and sphere records, the sphere -> owner
// references, pending added accelerations, persistent marks, and the current contact list with its history, re-keyed and re-sorted
// in the new numbering (it is the "previous list" of the detection that follows).  The caller's ids do not change.  Host-driven
// and not cheap (a second at 1e6 clumps, mostly host sorts): it is meant to happen every few ten thousand steps, not every detection.
static int order_apply(deme_ctx* c, const std::vector<uint32_t>& ord, const std::vector<OwnerRec>& ho, const std::vector<SphereRec>& hs);
static int order_renew(deme_ctx* c) {
    c->orderRenewDue = false;
    if (!c->orderEligible || c->arith != DEME_ARITH_FAST || c->nOwnerClumps <= 2 * (size_t)DEME_TILE_NB)
        return DEME_OK;  // (the exact mode keeps the caller's order: its sums are bit-identical to the oracle's only in that order)
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    const size_t nO = c->nOwners, nC = c->nOwnerClumps, nS = c->nSpheres;
    std::vector<OwnerRec> ho(nO);
    std::vector<SphereRec> hs(nS);
    HIPCK(hipMemcpyAsync(ho.data(), c->owners.p, nO * sizeof(OwnerRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(hs.data(), c->spheres.p, nS * sizeof(SphereRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<uint64_t> vox(nC);
    std::vector<uint16_t> lx(nC), ly(nC), lz(nC);
    for (size_t i = 0; i < nC; i++)
        vox[i] = ho[i].voxelID, lx[i] = ho[i].locX, ly[i] = ho[i].locY, lz[i] = ho[i].locZ;
    std::vector<uint32_t> ord;  // ord[k] = the CURRENT slot of the clump that goes to slot k
    double spread[2];
    order_compute(c->hp, nC, vox.data(), lx.data(), ly.data(), lz.data(), ord, spread);
    c->orderSpread[0] = spread[0], c->orderSpread[1] = spread[1];
    c->orderBaseHalo = 0, c->orderDetAt = c->nDetections;
    if (spread[0] <= 1.15 * spread[1])
        return DEME_OK;  // still as compact as a fresh order would be
    if (int rc = order_apply(c, ord, ho, hs))
        return rc;
    c->nOrderRenewals++;
    return DEME_OK;
}

// Back to the CALLER's order (deme_set_arith_mode(EXACT) on a context the engine had reordered): slot k takes the clump whose
// caller id is k; the maps become the identity and are dropped.
static int order_restore(deme_ctx* c) {
    c->orderRenewDue = false;
    if (!c->permuted)
        return DEME_OK;
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    const size_t nO = c->nOwners, nC = c->nOwnerClumps, nS = c->nSpheres;
    std::vector<OwnerRec> ho(nO);
    std::vector<SphereRec> hs(nS);
    HIPCK(hipMemcpyAsync(ho.data(), c->owners.p, nO * sizeof(OwnerRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(hs.data(), c->spheres.p, nS * sizeof(SphereRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> ord(nC);
    for (size_t k = 0; k < nC; k++)
        ord[k] = c->hE2O[k];
    if (int rc = order_apply(c, ord, ho, hs))
        return rc;
    // (order_apply composed the maps: they are the identity now)
    c->permuted = false;
    c->hO2E.clear(), c->hE2O.clear(), c->hS2E.clear(), c->hE2S.clear();
    c->dp.o2e = c->dp.s2e = nullptr;
    c->orderSpread[1] = c->orderSpread[0];
    return DEME_OK;
}

// Everything that is kept in engine slots follows the clumps to their new slots (ord[k] = the CURRENT slot of the clump that goes to
// slot k; ho / hs: the records as they stand).
static int order_apply(deme_ctx* c, const std::vector<uint32_t>& ord, const std::vector<OwnerRec>& ho, const std::vector<SphereRec>& hs) {
    const size_t nO = c->nOwners, nC = c->nOwnerClumps, nS = c->nSpheres;
    // slots: old -> new, owners and spheres
    std::vector<uint32_t> oOld2New(nO), sOld2New(nS), sNew2Old(nS);
    for (size_t k = 0; k < nC; k++)
        oOld2New[ord[k]] = (uint32_t)k;
    for (size_t k = nC; k < nO; k++)
        oOld2New[k] = (uint32_t)k;
    std::vector<uint32_t> first(nC + 1, 0);
    for (size_t i = 0; i < nS; i++)
        if (hs[i].owner < nC)
            first[hs[i].owner + 1]++;
    for (size_t i = 0; i < nC; i++)
        first[i + 1] += first[i];
    size_t w = 0;
    for (size_t k = 0; k < nC; k++)
        for (uint32_t e = first[ord[k]]; e < first[ord[k] + 1]; e++, w++)
            sNew2Old[w] = e, sOld2New[e] = (uint32_t)w;
    for (size_t i = first[nC]; i < nS; i++, w++)
        sNew2Old[w] = (uint32_t)i, sOld2New[i] = (uint32_t)i;
    // the caller's ids of the new slots
    const bool was = c->permuted;
    std::vector<uint32_t> o2e(nO), e2o(nO), s2e(nS), e2s(nS);
    for (size_t k = 0; k < nO; k++) {
        const uint32_t old = k < nC ? ord[k] : (uint32_t)k;
        o2e[k] = was ? c->hO2E[old] : old;
        e2o[o2e[k]] = (uint32_t)k;
    }
    for (size_t k = 0; k < nS; k++) {
        s2e[k] = was ? c->hS2E[sNew2Old[k]] : sNew2Old[k];
        e2s[s2e[k]] = (uint32_t)k;
    }
    // persistent marks: through the caller's ids (old maps still in place)
    for (auto& k : c->hPersist)
        k = order_key_out(c, k);
    // the current list, re-keyed (roles stay: they follow the caller's ids) and re-sorted, its history rows with it
    const size_t n = c->haveList ? c->nContacts : 0;
    const uint32_t nW = c->hp.nContactWildcards;
    std::vector<uint64_t> keys(n);
    std::vector<float> wcs(n * (size_t)std::max(nW, 1u));
    if (n) {
        HIPCK(hipMemcpyAsync(keys.data(), c->keysSorted[c->keysCur].p, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (nW)
            HIPCK(hipMemcpyAsync(wcs.data(), c->wc[c->wcCur].p, n * nW * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = keys[i];
        const uint32_t cls = key_class(k);
        keys[i] = make_key(cls, sOld2New[key_a(k)], cls == DEME_KEY_CLASS_SS ? sOld2New[key_b(k)] : key_b(k));
        perm[i] = (uint32_t)i;
    }
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint64_t> ks(n);
    std::vector<float> ws(wcs.size());
    for (size_t i = 0; i < n; i++) {
        ks[i] = keys[perm[i]];
        for (uint32_t q = 0; q < nW; q++)
            ws[i * nW + q] = wcs[(size_t)perm[i] * nW + q];
    }
    // records in their new slots
    std::vector<OwnerRec> no(nO);
    for (size_t k = 0; k < nO; k++)
        no[k] = ho[k < nC ? ord[k] : k];
    std::vector<SphereRec> ns(nS);
    for (size_t k = 0; k < nS; k++) {
        ns[k] = hs[sNew2Old[k]];
        ns[k].owner = oOld2New[ns[k].owner];
    }
    HIPCK(hipMemcpyAsync(c->owners.p, no.data(), nO * sizeof(OwnerRec), hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(c->spheres.p, ns.data(), nS * sizeof(SphereRec), hipMemcpyHostToDevice, c->stream));
    if (n) {
        HIPCK(hipMemcpyAsync(c->keysSorted[c->keysCur].p, ks.data(), n * 8, hipMemcpyHostToDevice, c->stream));
        if (nW)
            HIPCK(hipMemcpyAsync(c->wc[c->wcCur].p, ws.data(), n * nW * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!c->hNextAcc.empty()) {  // accelerations a script added for the coming step
        std::vector<AccRec> na(nO);
        for (size_t k = 0; k < nO; k++)
            na[k] = c->hNextAcc[k < nC ? ord[k] : k];
        c->hNextAcc.swap(na);
        HIPCK(hipMemcpyAsync(c->nextAcc.p, c->hNextAcc.data(), nO * sizeof(AccRec), hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    c->hO2E.swap(o2e), c->hE2O.swap(e2o), c->hS2E.swap(s2e), c->hE2S.swap(e2s);
    c->permuted = true;
    if (int rc = order_upload_maps(c))
        return rc;
    for (auto& k : c->hPersist)
        k = order_key_in(c, k);
    std::sort(c->hPersist.begin(), c->hPersist.end());
    if (!c->hPersist.empty())
        HIPCK(hipMemcpyAsync(c->persistKeys.p, c->hPersist.data(), c->hPersist.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    // what was built for the old slots
    c->list[c->cur].invalidate();
    c->conValid = false, c->conTile = false, c->fusedPrevValid = false;
    c->prescDirty = true;
    c->listStale = true;
    // The re-keyed list is a SEED of the detection that follows, not a list anything may be evaluated or downloaded from: the
    // per-contact and per-sphere products of the last detection (gather records, the history map, contact records, sphere
    // geometry) still sit in the old slots and row order.  deme_calc_forces refuses a seeded list and a step detects first; the
    // history map of a seed reads "no previous contact", contact records and sphere geometry are refused until that detection.
    if (c->haveList)
        c->seeded = true, c->nPrev = 0, c->mapFresh = false;
    c->geoStale = true;
    c->listSerial++;
    c->viewSerial = ~0ull;
    return DEME_OK;
}
