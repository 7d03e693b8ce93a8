// deme_decomp.inc -- the slab decomposition behind the C-ABI (SURVEY 8e; no reference equivalent: the reference splits kT / dT across
// two devices, DEM/APIPublic.cpp:22-72, and selects them in the constructor, DEM/API.h:52-56).  Included by deme_hip.hip inside its
// extern "C" block.  Three layers:
//   deme_decomp_*        the PLAN: a global scene cut into slabs along one axis -- equal-count cuts snapped to bin faces, own clumps,
//                        ghost sets, exchange lists, global ids.  Pure host code (no HIP call): a C++ host needs no numpy, and the
//                        CPU tests hold it against the numpy statement (dem-engine_amd/decomp.py: decompose).
//   deme_halo_group_build  the slabs of a plan that THIS rank holds become contexts of the group's device: parameters, scene,
//                        exchange lists (deme_halo_group_attach) and migration books (deme_halo_group_set_slab).
//   deme_multi_*         one process, several devices: a halo group per device (one RCCL rank each, communicators made in one
//                        grouped ncclCommInitRank), stepped by one host thread per device.  DEMSolver(nGPUs / device ids) sits on it.
// Scene order of a slab: [its own clumps | ghosts from the lower neighbour | ghosts from the upper neighbour | replicated owners].

struct DecompSlabPlan {
    // per owner of the slab
    std::vector<uint64_t> voxelID;
    std::vector<uint16_t> locX, locY, locZ, inertia;
    std::vector<float> qw, qx, qy, qz, vx, vy, vz, wx, wy, wz;
    std::vector<uint8_t> family, ghost;
    // per sphere
    std::vector<uint32_t> sphOwner;
    std::vector<uint16_t> sphComp, sphMat;
    // references into the slab's owner numbering
    std::vector<uint32_t> objOwner, ownerMesh;
    // books
    std::vector<uint32_t> ownerGlobal, sphereGlobal;  // global owner id per slab owner, global sphere id per slab sphere
    std::vector<uint32_t> sendLo, sendHi, recvLo, recvHi;  // LOCAL owner ids: sent to / taken from the lower / upper neighbour
    uint32_t nOwn = 0, nGhostLo = 0, nGhostHi = 0;
    double lo = 0, hi = 0;
    DemeScene scene{};
};

struct deme_decomp {
    uint32_t nSlabs = 0;
    int axis = 0;
    double halo = 0;
    std::vector<double> edges;  // nSlabs + 1; the outer two are -inf / +inf
    std::vector<DecompSlabPlan> slabs;
    std::vector<uint32_t> slabOfClump;  // which slab owns a clump of the global scene
    uint32_t nOwnersGlobal = 0, nClumpsGlobal = 0, nSpheresGlobal = 0;
    uint32_t nFree = 0;  // replicated owners that move under contact forces
};

namespace {

inline double decomp_coord(const DemeParams& p, uint64_t vox, uint16_t lx, uint16_t ly, uint16_t lz, int axis) {
    // the position decode of the kernels (deme_migrate.h: mig_world_coord): voxel * voxelSize + sub-voxel * l + LBF
    const uint64_t mx = ((uint64_t)1 << p.nvXp2) - 1, my = ((uint64_t)1 << p.nvYp2) - 1;
    if (axis == 0)
        return (double)(vox & mx) * p.voxelSize + (double)lx * p.l + (double)p.LBFX;
    if (axis == 1)
        return (double)((vox >> p.nvXp2) & my) * p.voxelSize + (double)ly * p.l + (double)p.LBFY;
    return (double)(vox >> (p.nvXp2 + p.nvYp2)) * p.voxelSize + (double)lz * p.l + (double)p.LBFZ;
}

template <class T>
inline void decomp_gather(std::vector<T>& dst, const T* src, const std::vector<uint32_t>& ids, T dflt) {
    dst.resize(ids.size());
    for (size_t i = 0; i < ids.size(); i++)
        dst[i] = src ? src[ids[i]] : dflt;
}

// largest distance from a clump's centre to the far side of one of its spheres
double decomp_max_reach(const DemeScene& s) {
    double reach = 0;
    for (uint32_t i = 0; i < s.nSpheres; i++) {
        if (s.ownerClumpBody[i] >= s.nOwnerClumps)
            continue;
        const uint32_t k = s.clumpComponentOffset[i];
        if (k >= s.nComp)
            continue;
        const double x = s.CDRelPosX[k], y = s.CDRelPosY[k], z = s.CDRelPosZ[k];
        reach = std::max(reach, std::sqrt(x * x + y * y + z * z) + (double)s.Radii[k]);
    }
    return reach;
}

int decomp_plan(const DemeParams& p, const DemeScene& s, uint32_t nSlabs, int axis, double halo, const double* edgesIn, uint32_t flags,
                deme_decomp& d, std::string& err) {
    char buf[512];
    if (nSlabs < 1 || axis > 2 || !s.voxelID || !s.locX || !s.locY || !s.locZ || (s.nSpheres && (!s.ownerClumpBody || !s.clumpComponentOffset))) {
        err = "deme_decomp_create: a scene with positions and clump-major spheres, and 1 or more slabs";
        return DEME_ERR_INVALID;
    }
    const uint32_t nC = s.nOwnerClumps, nO = s.nOwners, nS = s.nSpheres;
    for (uint32_t i = 1; i < nS; i++)
        if (s.ownerClumpBody[i] < s.ownerClumpBody[i - 1]) {
            err = "deme_decomp_create: spheres must be clump-major with ascending owners";
            return DEME_ERR_INVALID;
        }
    if (s.ownerGhost)
        for (uint32_t o = 0; o < nO; o++)
            if (s.ownerGhost[o] & 1u) {
                err = "deme_decomp_create: the scene to cut holds ghost copies already (it is a slab of a decomposition itself)";
                return DEME_ERR_INVALID;
            }
    // replicated owners that move under contact forces (decomp.py: `free`)
    std::vector<uint32_t> freeOwners;
    for (uint32_t o = nC; o < nO; o++) {
        const uint8_t f = s.familyID ? s.familyID[o] : 0;
        const uint8_t fl = s.familyFlags ? s.familyFlags[f] : 0;
        if (!(fl & (DEME_FAMILY_FIXED | DEME_FAMILY_PRESCRIBED)))
            freeOwners.push_back(o);
    }
    if (!freeOwners.empty() && !(flags & DEME_DECOMP_SHARED_FREE)) {
        snprintf(buf, sizeof(buf), "deme_decomp_create: replicated owner %u (a mesh / analytical body) moves under contact forces: pass "
                 "DEME_DECOMP_SHARED_FREE and step the slabs through a halo group, which adds its accelerations up across the slabs every step",
                 freeOwners[0]);
        err = buf;
        return DEME_ERR_INVALID;
    }
    // the axis: the longest side of the clumps' bounding box
    if (axis < 0) {
        double best = -1;
        for (int a = 0; a < 3; a++) {
            double lo = std::numeric_limits<double>::infinity(), hi = -lo;
            for (uint32_t o = 0; o < nC; o++) {
                const double v = decomp_coord(p, s.voxelID[o], s.locX[o], s.locY[o], s.locZ[o], a);
                lo = std::min(lo, v), hi = std::max(hi, v);
            }
            if (nC && hi - lo > best)
                best = hi - lo, axis = a;
        }
        if (axis < 0)
            axis = 0;
    }
    std::vector<double> x(nC);
    for (uint32_t o = 0; o < nC; o++)
        x[o] = decomp_coord(p, s.voxelID[o], s.locX[o], s.locY[o], s.locZ[o], axis);
    if (!(halo > 0)) {  // four clump reaches (a clump may drift two of them before the slabs are cut again) + the widest family margin
        double extra = 0;
        if (s.familyExtraMarginSize)
            for (int f = 0; f < 256; f++)
                extra = std::max(extra, (double)s.familyExtraMarginSize[f]);
        halo = 4.0 * decomp_max_reach(s) + 2.0 * extra;
    }
    d.nSlabs = nSlabs, d.axis = axis, d.halo = halo;
    d.nOwnersGlobal = nO, d.nClumpsGlobal = nC, d.nSpheresGlobal = nS, d.nFree = (uint32_t)freeOwners.size();
    const double inf = std::numeric_limits<double>::infinity();
    d.edges.assign(nSlabs + 1, 0.0);
    if (edgesIn) {
        for (uint32_t i = 0; i <= nSlabs; i++)
            d.edges[i] = edgesIn[i];
    } else {  // equal-count cuts (the quantiles of the clumps' coordinate, linear between order statistics) ...
        std::vector<double> xs(x);
        std::sort(xs.begin(), xs.end());
        const double lbf = axis == 0 ? (double)p.LBFX : axis == 1 ? (double)p.LBFY : (double)p.LBFZ;
        for (uint32_t i = 1; i < nSlabs; i++) {
            double e = 0;
            if (!xs.empty()) {
                const double pos = (double)i / (double)nSlabs * (double)(xs.size() - 1);
                const size_t k = (size_t)pos;
                e = k + 1 < xs.size() ? xs[k] + (xs[k + 1] - xs[k]) * (pos - (double)k) : xs.back();
            }
            if (!(flags & DEME_DECOMP_NO_SNAP) && p.binSize > 0)  // ... snapped to the nearest bin face (SURVEY 8e: bin-aligned slabs)
                e = lbf + std::nearbyint((e - lbf) / p.binSize) * p.binSize;
            d.edges[i] = e;
        }
    }
    d.edges[0] = -inf, d.edges[nSlabs] = inf;
    for (uint32_t i = 1; i <= nSlabs; i++)
        if (!(d.edges[i] >= d.edges[i - 1])) {
            err = "deme_decomp_create: the slab boundaries must ascend";
            return DEME_ERR_INVALID;
        }
    // ghosts are taken from the face neighbours only: an interior slab thinner than the halo would leave clumps of the slab after
    // next within reach of a face without a ghost copy
    for (uint32_t r = 1; r + 1 < nSlabs; r++)
        if (d.edges[r + 1] - d.edges[r] < halo) {
            snprintf(buf, sizeof(buf), "deme_decomp_create: slab %u is %.4g wide, thinner than the halo %.4g: use fewer slabs or a thinner halo", r,
                     d.edges[r + 1] - d.edges[r], halo);
            err = buf;
            return DEME_ERR_INVALID;
        }
    // owner slab of every clump: the last boundary that is <= x (numpy: searchsorted(edges, x, side="right") - 1, clipped)
    d.slabOfClump.resize(nC);
    for (uint32_t o = 0; o < nC; o++) {
        const uint32_t k = (uint32_t)(std::upper_bound(d.edges.begin(), d.edges.end(), x[o]) - d.edges.begin());
        d.slabOfClump[o] = std::min(std::max(k, 1u) - 1u, nSlabs - 1u);
    }
    std::vector<uint32_t> firstSphere(nO + 1, 0);  // spheres are clump-major
    for (uint32_t i = 0; i < nS; i++)
        firstSphere[s.ownerClumpBody[i] + 1]++;
    for (uint32_t o = 0; o < nO; o++)
        firstSphere[o + 1] += firstSphere[o];
    d.slabs.assign(nSlabs, DecompSlabPlan());
    // The order of a slab's clumps.  By default the global ids ascend (the numpy statement's order).  DEME_DECOMP_SPATIAL_ORDER: every
    // slab's OWN clumps are numbered the way the engine numbers an undivided scene (deme_order.inc: recursive bisection into
    // box-shaped owner tiles) -- a scene with ghosts keeps the order it is uploaded in, so a slab cut out of a sampler-ordered bed
    // would otherwise send most of its tiles through the per-tile fallback of the force pass -- and its ghosts follow the order their
    // owner slab gave them (a subsequence of a compact order; the exchange lists stay ascending on the sender's side).
    std::vector<uint32_t> slabRank(nC);
    for (uint32_t o = 0; o < nC; o++)
        slabRank[o] = o;
    if ((flags & DEME_DECOMP_SPATIAL_ORDER) && p.binSize > 0 && p.l > 0) {
        std::vector<std::vector<uint32_t>> members(nSlabs);
        for (uint32_t o = 0; o < nC; o++)
            members[d.slabOfClump[o]].push_back(o);
        for (uint32_t r = 0; r < nSlabs; r++) {
            const std::vector<uint32_t>& mem = members[r];
            if (mem.size() <= 2 * (size_t)DEME_TILE_NB)
                continue;
            std::vector<uint64_t> vv(mem.size());
            std::vector<uint16_t> ax(mem.size()), ay(mem.size()), az(mem.size());
            for (size_t i = 0; i < mem.size(); i++)
                vv[i] = s.voxelID[mem[i]], ax[i] = s.locX[mem[i]], ay[i] = s.locY[mem[i]], az[i] = s.locZ[mem[i]];
            std::vector<uint32_t> ord;
            double spread[2];
            order_compute(p, mem.size(), vv.data(), ax.data(), ay.data(), az.data(), ord, spread);
            if (spread[0] <= 1.15 * spread[1])
                continue;  // (compact as given: a bed the caller numbered along a curve)
            for (size_t k = 0; k < ord.size(); k++)
                slabRank[mem[ord[k]]] = (uint32_t)k;  // (ranks are compared inside one slab only)
        }
    }
    std::vector<uint32_t> newId(nO);
    for (uint32_t r = 0; r < nSlabs; r++) {
        DecompSlabPlan& q = d.slabs[r];
        q.lo = d.edges[r], q.hi = d.edges[r + 1];
        std::vector<uint32_t> own, gl, gr;
        for (uint32_t o = 0; o < nC; o++) {
            const uint32_t k = d.slabOfClump[o];
            if (k == r)
                own.push_back(o);
            else if (r > 0 && k == r - 1 && x[o] >= d.edges[r] - halo)
                gl.push_back(o);
            else if (r + 1 < nSlabs && k == r + 1 && x[o] < d.edges[r + 1] + halo)
                gr.push_back(o);
        }
        const auto byRank = [&](uint32_t a, uint32_t b) { return slabRank[a] < slabRank[b]; };
        std::sort(own.begin(), own.end(), byRank), std::sort(gl.begin(), gl.end(), byRank), std::sort(gr.begin(), gr.end(), byRank);
        q.nOwn = (uint32_t)own.size(), q.nGhostLo = (uint32_t)gl.size(), q.nGhostHi = (uint32_t)gr.size();
        std::vector<uint32_t>& og = q.ownerGlobal;
        og = own;
        og.insert(og.end(), gl.begin(), gl.end());
        og.insert(og.end(), gr.begin(), gr.end());
        const uint32_t nClHere = (uint32_t)og.size();
        for (uint32_t o = nC; o < nO; o++)
            og.push_back(o);
        std::fill(newId.begin(), newId.end(), 0xFFFFFFFFu);
        for (uint32_t i = 0; i < og.size(); i++)
            newId[og[i]] = i;
        decomp_gather(q.voxelID, s.voxelID, og, (uint64_t)0);
        decomp_gather(q.locX, s.locX, og, (uint16_t)0), decomp_gather(q.locY, s.locY, og, (uint16_t)0), decomp_gather(q.locZ, s.locZ, og, (uint16_t)0);
        decomp_gather(q.qw, s.oriQw, og, 1.f), decomp_gather(q.qx, s.oriQx, og, 0.f), decomp_gather(q.qy, s.oriQy, og, 0.f), decomp_gather(q.qz, s.oriQz, og, 0.f);
        decomp_gather(q.vx, s.vX, og, 0.f), decomp_gather(q.vy, s.vY, og, 0.f), decomp_gather(q.vz, s.vZ, og, 0.f);
        decomp_gather(q.wx, s.omgBarX, og, 0.f), decomp_gather(q.wy, s.omgBarY, og, 0.f), decomp_gather(q.wz, s.omgBarZ, og, 0.f);
        decomp_gather(q.family, s.familyID, og, (uint8_t)0);
        decomp_gather(q.inertia, s.inertiaPropOffsets, og, (uint16_t)0);
        q.ghost.assign(og.size(), 0);
        for (uint32_t i = q.nOwn; i < nClHere; i++)
            q.ghost[i] = 1;
        for (uint32_t o : freeOwners)
            q.ghost[newId[o]] = 2;  // summed across the slabs every step (DemeScene.ownerGhost)
        // spheres of the clumps held here, clump by clump
        size_t nSph = 0;
        for (uint32_t i = 0; i < nClHere; i++)
            nSph += firstSphere[og[i] + 1] - firstSphere[og[i]];
        q.sphereGlobal.reserve(nSph), q.sphOwner.reserve(nSph), q.sphComp.reserve(nSph), q.sphMat.reserve(nSph);
        for (uint32_t i = 0; i < nClHere; i++)
            for (uint32_t e = firstSphere[og[i]]; e < firstSphere[og[i] + 1]; e++) {
                q.sphereGlobal.push_back(e);
                q.sphOwner.push_back(i);
                q.sphComp.push_back(s.clumpComponentOffset[e]);
                q.sphMat.push_back(s.sphereMaterialOffset ? s.sphereMaterialOffset[e] : (uint16_t)0);
            }
        q.objOwner.resize(s.nAnal);
        for (uint32_t i = 0; i < s.nAnal; i++)
            q.objOwner[i] = newId[s.objOwner[i]];
        q.ownerMesh.resize(s.nTri);
        for (uint32_t i = 0; i < s.nTri; i++)
            q.ownerMesh[i] = newId[s.ownerMesh[i]];
        // what the neighbours hold as ghosts from here, in the neighbour's slot order (ascending global id on both sides)
        for (uint32_t i = 0; i < q.nOwn; i++) {
            if (r > 0 && x[own[i]] < d.edges[r] + halo)
                q.sendLo.push_back(i);
            if (r + 1 < nSlabs && x[own[i]] >= d.edges[r + 1] - halo)
                q.sendHi.push_back(i);
        }
        for (uint32_t i = 0; i < q.nGhostLo; i++)
            q.recvLo.push_back(q.nOwn + i);
        for (uint32_t i = 0; i < q.nGhostHi; i++)
            q.recvHi.push_back(q.nOwn + q.nGhostLo + i);
        // the slab's scene: its own per-owner / per-sphere arrays, the tables of the scene it was cut from
        DemeScene& t = q.scene;
        t = s;
        t.nOwners = (uint32_t)og.size(), t.nOwnerClumps = nClHere, t.nSpheres = (uint32_t)q.sphereGlobal.size();
        t.voxelID = q.voxelID.data(), t.locX = q.locX.data(), t.locY = q.locY.data(), t.locZ = q.locZ.data();
        t.oriQw = q.qw.data(), t.oriQx = q.qx.data(), t.oriQy = q.qy.data(), t.oriQz = q.qz.data();
        t.vX = q.vx.data(), t.vY = q.vy.data(), t.vZ = q.vz.data();
        t.omgBarX = q.wx.data(), t.omgBarY = q.wy.data(), t.omgBarZ = q.wz.data();
        t.familyID = q.family.data(), t.inertiaPropOffsets = q.inertia.data();
        t.ownerClumpBody = q.sphOwner.data(), t.clumpComponentOffset = q.sphComp.data(), t.sphereMaterialOffset = q.sphMat.data();
        t.objOwner = q.objOwner.data(), t.ownerMesh = s.nTri ? q.ownerMesh.data() : nullptr;
        // (a slab without ghost copies or summed replicas -- a plan of one slab -- is a plain scene: the engine may reorder it, §3.6)
        t.ownerGhost = std::any_of(q.ghost.begin(), q.ghost.end(), [](uint8_t g) { return g != 0; }) ? q.ghost.data() : nullptr;
    }
    // the exchange lists of two neighbours name the same clumps in the same order
    for (uint32_t r = 0; r + 1 < nSlabs; r++) {
        const DecompSlabPlan &a = d.slabs[r], &b = d.slabs[r + 1];
        bool ok = a.sendHi.size() == b.recvLo.size() && b.sendLo.size() == a.recvHi.size();
        for (size_t i = 0; ok && i < a.sendHi.size(); i++)
            ok = a.ownerGlobal[a.sendHi[i]] == b.ownerGlobal[b.recvLo[i]];
        for (size_t i = 0; ok && i < b.sendLo.size(); i++)
            ok = b.ownerGlobal[b.sendLo[i]] == a.ownerGlobal[a.recvHi[i]];
        if (!ok) {
            err = "deme_decomp_create: internal error -- the exchange lists of two neighbouring slabs disagree";
            return DEME_ERR_INVALID;
        }
    }
    return DEME_OK;
}

}  // namespace

int deme_decomp_create(const DemeParams* p, const DemeScene* scene, uint32_t nSlabs, int axis, double halo, const double* edges, uint32_t flags,
                       deme_decomp** out, char* err, size_t errCap) {
    if (err && errCap)
        err[0] = 0;
    if (!p || !scene || !out)
        return DEME_ERR_INVALID;
    *out = nullptr;
    deme_decomp* d = new deme_decomp();
    std::string msg;
    const int rc = decomp_plan(*p, *scene, nSlabs, axis, halo, edges, flags, *d, msg);
    if (rc != DEME_OK) {
        if (err && errCap)
            snprintf(err, errCap, "%s", msg.c_str());
        delete d;
        return rc;
    }
    *out = d;
    return DEME_OK;
}

void deme_decomp_destroy(deme_decomp* d) { delete d; }

int deme_decomp_info(const deme_decomp* d, uint32_t* nSlabs, int* axis, double* halo, double* edges, uint32_t* nFreeReplicated) {
    if (!d)
        return DEME_ERR_INVALID;
    if (nSlabs)
        *nSlabs = d->nSlabs;
    if (axis)
        *axis = d->axis;
    if (halo)
        *halo = d->halo;
    if (edges)
        for (uint32_t i = 0; i <= d->nSlabs; i++)
            edges[i] = d->edges[i];
    if (nFreeReplicated)
        *nFreeReplicated = d->nFree;
    return DEME_OK;
}

int deme_decomp_slab(const deme_decomp* d, uint32_t slab, DemeScene* scene, uint32_t counts[3], const uint32_t** ownerGlobal,
                     const uint32_t** sphereGlobal, const uint32_t** sendLower, uint32_t* nSendLower, const uint32_t** sendUpper,
                     uint32_t* nSendUpper, double range[2]) {
    if (!d || slab >= d->nSlabs)
        return DEME_ERR_INVALID;
    const DecompSlabPlan& q = d->slabs[slab];
    if (scene)
        *scene = q.scene;
    if (counts)
        counts[0] = q.nOwn, counts[1] = q.nGhostLo, counts[2] = q.nGhostHi;
    if (ownerGlobal)
        *ownerGlobal = q.ownerGlobal.data();
    if (sphereGlobal)
        *sphereGlobal = q.sphereGlobal.data();
    if (sendLower)
        *sendLower = q.sendLo.data();
    if (nSendLower)
        *nSendLower = (uint32_t)q.sendLo.size();
    if (sendUpper)
        *sendUpper = q.sendHi.data();
    if (nSendUpper)
        *nSendUpper = (uint32_t)q.sendHi.size();
    if (range)
        range[0] = q.lo, range[1] = q.hi;
    return DEME_OK;
}

// ---- the slabs of a plan on the devices -----------------------------------------------------------------------------------------
int deme_halo_group_set_axis(deme_halo_group* g, int axis) {
    if (!g || axis < 0 || axis > 2)
        return DEME_ERR_INVALID;
    g->axis = axis;
    return DEME_OK;
}

int deme_halo_group_num_slabs(const deme_halo_group* g, uint32_t* n) {
    if (!g || !n)
        return DEME_ERR_INVALID;
    *n = (uint32_t)g->slabs.size();
    return DEME_OK;
}

int deme_halo_group_slab_ctx(deme_halo_group* g, uint32_t i, deme_ctx** ctx, uint32_t* globalSlab) {
    if (!g || !ctx || i >= g->slabs.size())
        return DEME_ERR_INVALID;
    *ctx = g->slabs[i].ctx;
    if (globalSlab)
        *globalSlab = g->firstSlab + i;
    return DEME_OK;
}

int deme_halo_group_build(deme_halo_group* g, const DemeParams* p, const deme_decomp* plan, int arith, uint32_t flipMask) {
    if (!g || !g->comm || !p || !plan)
        return DEME_ERR_INVALID;
    if (!g->slabs.empty())
        return gfail(g, DEME_ERR_INVALID, "build: the group holds slabs already");
    if (plan->nSlabs % (uint32_t)g->world)
        return gfail(g, DEME_ERR_INVALID, "build: %u slabs do not divide among %d ranks", plan->nSlabs, g->world);
    GHIP(hipSetDevice(g->device));
    const uint32_t per = plan->nSlabs / (uint32_t)g->world, first = (uint32_t)g->rank * per;
    g->axis = plan->axis, g->firstSlab = first;
    std::vector<deme_ctx*> ctxs(per, nullptr);
    for (uint32_t i = 0; i < per; i++) {
        deme_ctx* c = nullptr;
        if (int rc = deme_ctx_create(g->device, &c))
            return gfail(g, rc, "build: deme_ctx_create on device %d failed", g->device);
        g->ownedCtx.push_back(c);
        ctxs[i] = c;
        if (arith >= 0)
            if (int rc = deme_set_arith_mode(c, arith))
                return gfail(g, rc, "build: arithmetic mode %d", arith);
        if (int rc = deme_set_params(c, p))
            return gfail(g, rc, "build (slab %u, parameters): %s", first + i, c->err.c_str());
        if (int rc = deme_upload_scene(c, &plan->slabs[first + i].scene))
            return gfail(g, rc, "build (slab %u, scene): %s", first + i, c->err.c_str());
    }
    for (uint32_t i = 0; i < per; i++) {
        const uint32_t sl = first + i;
        const DecompSlabPlan& q = plan->slabs[sl];
        // the neighbour of a face: a slab of this rank (its context), of another rank, or nobody at the ends of the chain
        const int loRank = sl == 0 ? -1 : (int)((sl - 1) / per), hiRank = sl + 1 >= plan->nSlabs ? -1 : (int)((sl + 1) / per);
        deme_ctx* loCtx = (loRank == g->rank) ? ctxs[i - 1] : nullptr;
        deme_ctx* hiCtx = (hiRank == g->rank) ? ctxs[i + 1] : nullptr;
        if (int rc = deme_halo_group_attach(g, ctxs[i], loRank, loCtx, q.sendLo.data(), (uint32_t)q.sendLo.size(), q.recvLo.data(),
                                            (uint32_t)q.recvLo.size(), hiRank, hiCtx, q.sendHi.data(), (uint32_t)q.sendHi.size(), q.recvHi.data(),
                                            (uint32_t)q.recvHi.size()))
            return rc;
        if (int rc = deme_halo_group_set_slab(g, ctxs[i], q.ownerGlobal.data(), q.sphereGlobal.data(), q.nOwn, q.nGhostLo, q.nGhostHi, q.lo, q.hi,
                                              plan->halo, flipMask))
            return rc;
    }
    g->nOwnersGlobal = plan->nOwnersGlobal, g->nClumpsGlobal = plan->nClumpsGlobal;
    return DEME_OK;  // (the ghost copies were uploaded with their owners' state: no exchange is needed before the first step)
}

namespace {
// one slab as the host code of a decomposed run walks it
struct SlabRef {
    deme_halo_group* g;
    HaloSlab* s;
    deme_ctx* c;
    uint32_t no;  // its number in the whole chain
    bool first;   // the first slab of the chain: the one that answers for the replicated owners
};
inline SlabRef slab_ref(deme_halo_group* g, size_t k) { return {g, &g->slabs[k], g->slabs[k].ctx, g->firstSlab + (uint32_t)k, g->firstSlab + k == 0}; }
// WHO REPORTS A ROW that is read by global id: an own clump's comes from its slab, a replicated owner's from the first slab of the
// chain, a ghost copy's from nobody (its owner slab reports it).  k_query_owner_state (deme_query.h) applies the same rule on the device.
inline bool slab_reports(const SlabRef& r, uint32_t ownerSlot) { return ownerSlot < r.s->geo.nOwn || (ownerSlot >= r.c->nOwnerClumps && r.first); }
// WHO TAKES A ROW that is added once per owner (deme_multi_add_owner_acc): own clumps and replicated owners, on every slab.  (State
// written by global id goes to every copy, ghosts included: rows_in, k_scatter_owner_state.)
inline bool slab_takes(const SlabRef& r, uint32_t ownerSlot) { return ownerSlot < r.s->geo.nOwn || ownerSlot >= r.c->nOwnerClumps; }
// the rows a slab reports, from the slab's arrays to the caller's arrays of the global scene
template <class T>
inline void rows_out(T* dst, const T* src, const std::vector<uint32_t>& gid, const SlabRef& r) {
    if (!dst || !src)
        return;
    for (size_t i = 0; i < gid.size(); i++)
        if (slab_reports(r, (uint32_t)i))
            dst[gid[i]] = src[i];
}
template <class T>
inline void rows_in(T* dst, const T* src, const std::vector<uint32_t>& gid) {
    if (!dst || !src)
        return;
    for (size_t i = 0; i < gid.size(); i++)  // ghosts and replicated owners included: every copy takes the caller's value
        dst[i] = src[gid[i]];
}
struct OwnerStateBuf {  // host room for every column of n owners, named by st
#define DEME_COL(abi, T, Rec, f) std::vector<T> abi;
    DEME_OWNER_COLS(DEME_COL, DEME_COL, DEME_COL)
#undef DEME_COL
    DemeOwnerState st{};
    explicit OwnerStateBuf(size_t n) {
#define DEME_COL(abi, T, Rec, f) abi.resize(n), st.abi = abi.data();
        DEME_OWNER_COLS(DEME_COL, DEME_COL, DEME_COL)
#undef DEME_COL
    }
};
}  // namespace

static int group_state_io(deme_halo_group* g, DemeOwnerState* glob, uint32_t nOwnersGlobal, bool down) {
    if (!g || !glob)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    for (size_t k = 0; k < g->slabs.size(); k++) {
        const SlabRef r = slab_ref(g, k);
        HaloSlab& s = *r.s;
        deme_ctx* c = r.c;
        if (!s.geo.set)
            return gfail(g, DEME_ERR_INVALID, "state by global id: slab %zu has no books (deme_halo_group_set_slab / _build)", k);
        std::vector<uint32_t> gid(c->nOwners);
        GHIP(hipStreamSynchronize(c->stream));
        GHIP(slab_ids_host(s, gid.data(), nullptr, nullptr, nullptr));
        for (size_t i = 0; i < gid.size(); i++)
            if (gid[i] >= nOwnersGlobal)
                return gfail(g, DEME_ERR_INVALID, "state by global id: owner id %u beyond the %u rows given (slab %zu, slot %zu of %u owners: %u own, %u + %u ghosts, %u clumps)",
                             gid[i], nOwnersGlobal, k, i, c->nOwners, s.geo.nOwn, s.geo.nGL, s.geo.nGR, c->nOwnerClumps);
        OwnerStateBuf b(std::max<size_t>(c->nOwners, 1));
        if (down) {
            if (int rc = deme_download_owner_state(c, &b.st))
                return gfail(g, rc, "state by global id (slab %zu): %s", k, c->err.c_str());
#define DEME_COL(abi, T, Rec, f) rows_out(glob->abi, (const T*)b.st.abi, gid, r);
            DEME_OWNER_COLS(DEME_COL, DEME_COL, DEME_COL)
#undef DEME_COL
        } else {
            DemeOwnerState up{};  // (a / alpha are not written by global id)
#define DEME_COL(abi, T, Rec, f) \
    if (glob->abi)               \
        rows_in(b.st.abi, (const T*)glob->abi, gid), up.abi = b.st.abi;
            DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL)
#undef DEME_COL
            if (int rc = deme_upload_owner_state(c, &up))
                return gfail(g, rc, "state by global id (slab %zu): %s", k, c->err.c_str());
        }
    }
    return DEME_OK;
}
int deme_halo_group_download_state(deme_halo_group* g, DemeOwnerState* glob, uint32_t nOwnersGlobal) { return group_state_io(g, glob, nOwnersGlobal, true); }
int deme_halo_group_upload_state(deme_halo_group* g, const DemeOwnerState* glob, uint32_t nOwnersGlobal) {
    return group_state_io(g, const_cast<DemeOwnerState*>(glob), nOwnersGlobal, false);
}

// ---- one process, several devices ------------------------------------------------------------------------------------------------
// one row of the merged contact list of a decomposed run (deme_multi_download_contacts, below)
struct MultiRow {
    uint64_t key;  // A << 34 | class << 31 | B  (class: 0 sphere-sphere, 1 sphere-mesh, 2 sphere-analytical: make_key's order)
    uint32_t slab, row;
    uint8_t type, flipped;
};
// One host thread per device that lives as long as the run (round 6; multi_each spawned and joined a std::thread per device on every
// deme_multi_step / migrate / sync call: a script that calls DoDynamics in frame-sized pieces paid thread creation and RCCL's
// per-thread set-up each time).  A worker selects its device once, then runs the jobs it is handed, one at a time.
struct MultiWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    int rc = DEME_OK;
    bool pending = false, quit = false;
    explicit MultiWorker(int device) {
        th = std::thread([this, device]() {
            hipSetDevice(device);
            std::unique_lock<std::mutex> lk(mu);
            for (;;) {
                cv.wait(lk, [&] { return pending || quit; });
                if (quit)
                    return;
                lk.unlock();
                const int r = job();
                lk.lock();
                rc = r, pending = false;
                cv.notify_all();
            }
        });
    }
    void post(std::function<int()> f) {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(f), pending = true;
        cv.notify_all();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !pending; });
        return rc;
    }
    ~MultiWorker() {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
            cv.notify_all();
        }
        if (th.joinable())
            th.join();
    }
};
struct deme_multi {
    std::vector<int> devices;
    std::vector<std::unique_ptr<MultiWorker>> workers;  // one per device once a call has gone to several (multi_each)
    std::vector<deme_halo_group*> groups;  // one per device: RCCL rank i of a communicator that spans the devices
    deme_decomp* plan = nullptr;
    uint32_t migrateEvery = 0, sinceMigration = 0;
    uint32_t rebalanceEvery = 0, migrationsSinceRebalance = 0;  // every n-th due migration recomputes the boundaries first
    uint64_t nRebalances = 0;
    uint64_t clumpsMigrated = 0, nSteps = 0;
    std::vector<MultiRow> rows;  // the merged list, built on demand and kept until the next step / upload
    uint64_t rowsAtStep = 0;
    bool rowsValid = false;
    uint64_t qHostBytes = 0;  // bytes the by-owner queries have copied to the host (deme_multi_query_host_bytes)
    std::string err;
    bool said = false;  // mfail has written err since multi_slabs last asked
};

int deme_scene_sizes(const deme_ctx* c, uint32_t out[4]) {
    if (!c || !out)
        return DEME_ERR_INVALID;
    out[0] = c->nOwners, out[1] = c->nOwnerClumps, out[2] = c->nSpheres, out[3] = c->hp.nContactWildcards;
    return DEME_OK;
}

int deme_device_count(int* n) {
    if (!n)
        return DEME_ERR_INVALID;
    int k = 0;
    if (hipGetDeviceCount(&k) != hipSuccess)
        k = 0;  // (no driver / no device: zero visible devices, not an error of this call)
    *n = k;
    return DEME_OK;
}

namespace {
int mfail(deme_multi* m, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (m)
        m->err = buf, m->said = true;
    return code;
}
// the same call on every group: inline for one device, one host thread per device otherwise (each group's loop is written as the
// loop of a process of its own -- RCCL calls of one communicator wait for the peers' calls, which another thread issues)
template <class F>
int multi_each(deme_multi* m, F f) {
    const size_t n = m->groups.size();
    std::vector<int> rc(n, DEME_OK);
    static const bool forceWorkers = getenv("DEME_MULTI_FORCE_WORKERS") && atoi(getenv("DEME_MULTI_FORCE_WORKERS"));  // (tests: the worker path on one device)
    if (n == 1 && !forceWorkers) {
        rc[0] = f(m->groups[0], (size_t)0);
    } else {
        if (m->workers.size() != n) {
            m->workers.clear();
            for (size_t i = 0; i < n; i++)
                m->workers.emplace_back(new MultiWorker(m->devices[i]));
        }
        for (size_t i = 0; i < n; i++)
            m->workers[i]->post([&f, m, i]() { return f(m->groups[i], i); });
        for (size_t i = 0; i < n; i++)
            rc[i] = m->workers[i]->wait();
    }
    for (size_t i = 0; i < n; i++)
        if (rc[i] != DEME_OK && rc[i] != DEME_ERR_PEER)
            return mfail(m, rc[i], "device %d: %s", m->devices[i], deme_halo_group_last_error(m->groups[i]));
    for (size_t i = 0; i < n; i++)
        if (rc[i] != DEME_OK)
            return mfail(m, rc[i], "device %d: %s", m->devices[i], deme_halo_group_last_error(m->groups[i]));
    return DEME_OK;
}
// The host's walk over the slabs, one after the other in the order of the chain: f(const SlabRef&) -> int, each group's device
// selected once.  A non-zero return ends the walk; unless f has said why through mfail, the message of the slab's context is the run's.
template <class F>
int multi_slabs(deme_multi* m, F f) {
    for (auto* g : m->groups) {
        if (hipSetDevice(g->device) != hipSuccess)
            return mfail(m, DEME_ERR_HIP, "device %d cannot be selected", g->device);
        for (size_t k = 0; k < g->slabs.size(); k++) {
            const SlabRef r = slab_ref(g, k);
            m->said = false;
            if (int rc = f(r))
                return m->said ? rc : mfail(m, rc, "%s", r.c->err.c_str());
        }
    }
    return DEME_OK;
}
// slab number slabNo of the chain (c == null: the run holds no such slab); no device is selected
SlabRef multi_slab(const deme_multi* m, uint32_t slabNo) {
    const uint32_t per = m->plan->nSlabs / (uint32_t)m->groups.size();
    deme_halo_group* g = slabNo < m->plan->nSlabs ? m->groups[slabNo / per] : nullptr;
    return g && slabNo % per < g->slabs.size() ? slab_ref(g, slabNo % per) : SlabRef{g, nullptr, nullptr, slabNo, false};
}
// a slab's id books on the host (slab_ids_host), only the arrays `what` names, inside a walk of multi_slabs
enum : unsigned { IDS_OWNER = 1, IDS_SPHERE = 2, IDS_SPHERE_OWNER = 4 };
struct SlabIds {
    std::vector<uint32_t> ownerGid, sphereGid, sphereOwner;  // owner slot -> global id, sphere -> global id, sphere -> owner slot
};
int slab_ids(deme_multi* m, const SlabRef& r, unsigned what, SlabIds& b) {
    b.ownerGid.resize(what & IDS_OWNER ? r.c->nOwners : 0), b.sphereGid.resize(what & IDS_SPHERE ? r.c->nSpheres : 0);
    b.sphereOwner.resize(what & IDS_SPHERE_OWNER ? r.c->nSpheres : 0);
    if (slab_ids_host(*r.s, what & IDS_OWNER ? b.ownerGid.data() : nullptr, what & IDS_SPHERE ? b.sphereGid.data() : nullptr,
                      what & IDS_SPHERE_OWNER ? b.sphereOwner.data() : nullptr, nullptr) != hipSuccess)
        return mfail(m, DEME_ERR_HIP, "the slab's books could not be read");
    return DEME_OK;
}
// what deme_multi_download_contact_records would say of a slab (a slab with an empty list is not asked)
inline int slab_records_refused(const SlabRef& r) { return r.c->nContacts ? records_refused(r.c) : DEME_OK; }
}  // namespace

// one halo group per device of m->devices: a group of its own for one device, one communicator over several (every rank's
// ncclCommInitRank inside one RCCL group: the single-process form, one thread per rank since each call waits for the others)
static int multi_open_groups(deme_multi* m) {
    const int nDevices = (int)m->devices.size();
    m->groups.assign(nDevices, nullptr);
    int rc = DEME_OK;
    if (nDevices == 1) {
        rc = deme_halo_group_create(nullptr, 0, 1, m->devices[0], &m->groups[0]);
    } else {
        unsigned char id[128];
        rc = deme_halo_unique_id(id);
        if (rc == DEME_OK) {
            std::vector<int> rcs(nDevices, DEME_OK);
            std::vector<std::thread> th;
            for (int i = 0; i < nDevices; i++)
                th.emplace_back([&, i]() { rcs[i] = deme_halo_group_create(id, i, nDevices, m->devices[i], &m->groups[i]); });
            for (auto& t : th)
                t.join();
            for (int i = 0; i < nDevices && rc == DEME_OK; i++)
                rc = rcs[i];
        }
    }
    if (rc != DEME_OK) {
        m->err = "the halo groups could not be opened";
        for (auto* g : m->groups)
            if (g && deme_halo_group_last_error(g)[0]) {
                m->err = deme_halo_group_last_error(g);
                break;
            }
    }
    return rc;
}

int deme_multi_create(const int* devices, int nDevices, deme_multi** out, char* err, size_t errCap) {
    auto say = [&](const char* fmt, ...) {
        if (err && errCap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(err, errCap, fmt, ap);
            va_end(ap);
        }
    };
    if (err && errCap)
        err[0] = 0;
    if (!out)
        return DEME_ERR_INVALID;
    *out = nullptr;
    if (!devices || nDevices < 1) {
        say("deme_multi_create: at least one device id");
        return DEME_ERR_INVALID;
    }
    int visible = 0;
    deme_device_count(&visible);
    for (int i = 0; i < nDevices; i++) {
        if (devices[i] < 0 || devices[i] >= visible) {  // GpuManager.cpp:64-68: the reference throws when it cannot have the devices it was asked for
            say("deme_multi_create: device id %d is not present (%d HIP device%s visible)", devices[i], visible, visible == 1 ? "" : "s");
            return DEME_ERR_INVALID;
        }
        for (int j = 0; j < i; j++)
            if (devices[j] == devices[i]) {
                say("deme_multi_create: device id %d is given twice (one RCCL rank per device)", devices[i]);
                return DEME_ERR_INVALID;
            }
    }
    deme_multi* m = new deme_multi();
    m->devices.assign(devices, devices + nDevices);
    const int rc = multi_open_groups(m);
    if (rc != DEME_OK) {
        if (err && errCap)
            snprintf(err, errCap, "deme_multi_create: %s", m->err.empty() ? "the halo groups could not be opened" : m->err.c_str());
        deme_multi_destroy(m);
        return rc;
    }
    *out = m;
    return DEME_OK;
}

void deme_multi_destroy(deme_multi* m) {
    if (!m)
        return;
    m->workers.clear();  // (joins the device threads)
    for (auto* g : m->groups)
        if (g)
            deme_halo_group_destroy(g);
    if (m->plan)
        deme_decomp_destroy(m->plan);
    delete m;
}

// back to the state after deme_multi_create: the slabs, their contexts and the plan are dropped, the devices' groups opened anew
// (communicators included: a scene is re-uploaded a few times in a run at most -- UpdateClumps, ResortClumps).  deme_multi_build follows.
int deme_multi_reset(deme_multi* m) {
    if (!m)
        return DEME_ERR_INVALID;
    for (auto*& g : m->groups)
        if (g) {
            deme_halo_group_destroy(g);
            g = nullptr;
        }
    if (m->plan)
        deme_decomp_destroy(m->plan);
    m->plan = nullptr;
    m->sinceMigration = 0, m->migrationsSinceRebalance = 0, m->rows.clear(), m->rowsValid = false;
    return multi_open_groups(m);
}

const char* deme_multi_last_error(const deme_multi* m) { return m ? m->err.c_str() : "null deme_multi"; }

int deme_multi_build(deme_multi* m, const DemeParams* p, const DemeScene* scene, uint32_t slabsPerDevice, int axis, double halo, uint32_t flags,
                     int arith, uint32_t flipMask) {
    if (!m || !p || !scene || slabsPerDevice < 1)
        return DEME_ERR_INVALID;
    if (m->plan)
        return mfail(m, DEME_ERR_INVALID, "deme_multi_build: built already");
    char msg[512];
    const uint32_t nSlabs = slabsPerDevice * (uint32_t)m->groups.size();
    if (nSlabs > 1 && !(flags & DEME_DECOMP_CALLER_ORDER))
        flags |= DEME_DECOMP_SPATIAL_ORDER;  // (slabs keep the order they are uploaded in: give them the engine's)
    if (int rc = deme_decomp_create(p, scene, nSlabs, axis, halo, nullptr, flags, &m->plan, msg, sizeof(msg)))
        return mfail(m, rc, "%s", msg);
    if (m->plan->nSpheresGlobal >= (1ull << 30)) {  // (the merged contact list's keys hold a global sphere id in 30 bits: multi_contact_rows)
        deme_decomp_destroy(m->plan), m->plan = nullptr;
        return mfail(m, DEME_ERR_INVALID, "deme_multi_build: %llu spheres; a decomposed run's merged contact list numbers at most 2^30 - 1",
                     (unsigned long long)scene->nSpheres);
    }
    return multi_each(m, [&](deme_halo_group* g, size_t) { return deme_halo_group_build(g, p, m->plan, arith, flipMask); });
}

int deme_multi_num_slabs(const deme_multi* m, uint32_t* n) {
    if (!m || !n)
        return DEME_ERR_INVALID;
    *n = m->plan ? m->plan->nSlabs : 0u;
    return DEME_OK;
}

int deme_multi_slab_ctx(deme_multi* m, uint32_t slab, deme_ctx** ctx) {
    if (int rc = deme_multi_slab_ctx_peek(m, slab, const_cast<const deme_ctx**>(ctx)))
        return rc;
    m->rowsValid = false;  // (the caller may change what the slab lists: the merged contact list is rebuilt on its next use)
    return DEME_OK;
}

// ... for questions that change nothing (kernel names, bin size, timers): the merged contact list stays valid
int deme_multi_slab_ctx_peek(const deme_multi* m, uint32_t slab, const deme_ctx** ctx) {
    if (!m || !ctx || !m->plan)
        return DEME_ERR_INVALID;
    *ctx = multi_slab(m, slab).c;
    return *ctx ? DEME_OK : DEME_ERR_INVALID;
}

int deme_multi_set_migration(deme_multi* m, uint32_t migrateEvery) {
    if (!m)
        return DEME_ERR_INVALID;
    m->migrateEvery = migrateEvery;
    return DEME_OK;
}

int deme_multi_step(deme_multi* m, uint32_t nsteps) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const bool single = m->plan->nSlabs == 1;  // one slab on one device: nothing to exchange, nothing to migrate
    while (nsteps) {
        uint32_t n = nsteps;
        if (m->migrateEvery && !single)
            n = std::min(n, m->migrateEvery - std::min(m->sinceMigration, m->migrateEvery - 1u));
        if (int rc = multi_each(m, [&](deme_halo_group* g, size_t) { return deme_halo_group_step(g, n); }))
            return rc;
        nsteps -= n, m->nSteps += n, m->sinceMigration += n;
        if (m->migrateEvery && !single && m->sinceMigration >= m->migrateEvery) {
            if (m->rebalanceEvery && ++m->migrationsSinceRebalance >= m->rebalanceEvery) {
                if (int rc = deme_multi_rebalance(m, nullptr, nullptr))  // (boundaries recomputed, then the same migration)
                    return rc;
                continue;
            }
            std::vector<uint32_t> moved(m->groups.size(), 0);
            if (int rc = multi_each(m, [&](deme_halo_group* g, size_t i) { return deme_halo_group_migrate(g, &moved[i]); }))
                return rc;
            for (uint32_t v : moved)
                m->clumpsMigrated += v;
            m->sinceMigration = 0;
        }
    }
    return DEME_OK;
}

int deme_multi_set_rebalance(deme_multi* m, uint32_t everyNthMigration) {
    if (!m)
        return DEME_ERR_INVALID;
    m->rebalanceEvery = everyNthMigration, m->migrationsSinceRebalance = 0;
    return DEME_OK;
}

int deme_multi_sync(deme_multi* m) {
    if (!m)
        return DEME_ERR_INVALID;
    return multi_each(m, [&](deme_halo_group* g, size_t) { return deme_halo_group_sync(g); });
}

int deme_multi_download_state(deme_multi* m, DemeOwnerState* glob, uint32_t nOwnersGlobal) {
    if (!m || !glob || !m->plan)
        return DEME_ERR_INVALID;
    for (size_t i = 0; i < m->groups.size(); i++)  // (host-side scatter into the caller's arrays: one group after the other)
        if (int rc = deme_halo_group_download_state(m->groups[i], glob, nOwnersGlobal))
            return mfail(m, rc, "device %d: %s", m->devices[i], deme_halo_group_last_error(m->groups[i]));
    return DEME_OK;
}

int deme_multi_upload_state(deme_multi* m, const DemeOwnerState* glob, uint32_t nOwnersGlobal) {
    if (!m || !glob || !m->plan)
        return DEME_ERR_INVALID;
    m->rowsValid = false;
    for (size_t i = 0; i < m->groups.size(); i++)
        if (int rc = deme_halo_group_upload_state(m->groups[i], glob, nOwnersGlobal))
            return mfail(m, rc, "device %d: %s", m->devices[i], deme_halo_group_last_error(m->groups[i]));
    return DEME_OK;
}

int deme_multi_counts(deme_multi* m, DemeCounts* sum, uint64_t* clumpsMigrated) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (sum) {
        *sum = DemeCounts{};
        if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
                DemeCounts c{};
                if (int rc = deme_get_counts(r.c, &c))
                    return rc;
                sum->nContacts += c.nContacts, sum->nPrevContacts += c.nPrevContacts, sum->nBinSphereTouches += c.nBinSphereTouches;
                sum->nActiveBins += c.nActiveBins;
                sum->maxSpheresInBin = std::max(sum->maxSpheresInBin, c.maxSpheresInBin);
                if (r.first)
                    sum->nSteps = c.nSteps, sum->nDetections = c.nDetections;
                if (c.lastStatus)
                    sum->lastStatus = c.lastStatus;
                return DEME_OK;
            }))
            return rc;
    }
    if (clumpsMigrated)
        *clumpsMigrated = m->clumpsMigrated;
    return DEME_OK;
}


// ---- measurement aid: the HBM rate a hand-written streaming copy reaches on this device (SURVEY 8d: "measure the attainable peak on the
// box with a streaming copy kernel and quote both").  16 bytes per lane and trip, grid-stride, `bytes` read + `bytes` written.
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = src[i];
}
// ... four loads in flight per lane, streaming (non-temporal) loads and stores: the form the guide's 6.29 TB/s figure is quoted for
typedef uint32_t copy_v4u __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_copy16x4(const copy_v4u* __restrict__ src, copy_v4u* __restrict__ dst, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        const copy_v4u a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride),
                       c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
        __builtin_nontemporal_store(a, dst + i), __builtin_nontemporal_store(b, dst + i + stride);
        __builtin_nontemporal_store(c, dst + i + 2 * stride), __builtin_nontemporal_store(d, dst + i + 3 * stride);
    }
    for (; i < n; i += stride)
        dst[i] = src[i];
}
int deme_copy_rate_probe(int device, size_t bytes, int reps, double* GBs) {
    if (!GBs || bytes < (1u << 20) || reps < 1)
        return DEME_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess)
        return DEME_ERR_HIP;
    void *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = DEME_ERR_HIP;
    double best = 0;
    const size_t n = bytes / 16;
    if (hipMalloc(&a, n * 16) == hipSuccess && hipMalloc(&b, n * 16) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
        hipEventCreate(&e1) == hipSuccess && hipMemset(a, 1, n * 16) == hipSuccess) {
        rc = DEME_OK;
        // the best of: plain / four-in-flight streaming form, 8 / 16 / 32 workgroups per CU
        for (int r = 0; r <= 6 * reps && rc == DEME_OK; r++) {  // (the first trip warms up)
            const int form = r % 2, wg = 8 << ((r / 2) % 3);
            hipEventRecord(e0, nullptr);
            if (form == 0)
                hipLaunchKernelGGL(k_copy16, dim3(256 * wg), dim3(256), 0, nullptr, (const uint4*)a, (uint4*)b, n);
            else
                hipLaunchKernelGGL(k_copy16x4, dim3(256 * wg), dim3(256), 0, nullptr, (const copy_v4u*)a, (copy_v4u*)b, n);
            hipEventRecord(e1, nullptr);
            float ms = 0;
            if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess)
                rc = DEME_ERR_HIP;
            else if (r > 0 && ms > 0)
                best = std::max(best, 2.0 * (double)(n * 16) / ((double)ms * 1e-3) / 1e9);
        }
    }
    if (e0)
        hipEventDestroy(e0);
    if (e1)
        hipEventDestroy(e1);
    if (a)
        hipFree(a);
    if (b)
        hipFree(b);
    *GBs = best;
    return rc;
}

// ---- the contact list of a decomposed run, in GLOBAL sphere ids ---------------------------------------------------------------------
// Every slab lists its contacts in its own numbering; a contact between an own clump and a ghost is on two slabs' lists (unless
// deme_halo_group_set_cross_contacts(1)).  The merged list reports a pair ONCE -- by the slab that owns the clump of the globally
// smaller sphere (sphere-analytical / sphere-mesh pairs go with sphere A's clump: decomp.py, _globalise_pairs) --, sphere-sphere
// pairs as (smaller, larger) global id, rows in the canonical order of an undivided context (A, class, B).  A pair whose slab had it
// the other way round is FLIPPED: its B -> A vector wildcards (flipMask) and its recorded force change sign, its contact points swap.
namespace {
// A pair in GLOBAL ids as the merged list names it: a sphere-sphere pair smaller id first (flipped: it was given the other way
// round), the key in the list's order (A, class, B).  k_query_select (deme_query.h) builds the same on the device.
struct GlobalPair {
    uint64_t key;
    uint32_t a, b;
    bool flipped;
};
inline GlobalPair global_pair(uint32_t gA, uint32_t gB, uint8_t type) {
    const bool flipped = type == DEME_SPHERE_SPHERE_CONTACT && gA > gB;
    if (flipped)
        std::swap(gA, gB);
    return {merged_key(key_class_of_type(type), gA, gB), gA, gB, flipped};
}
// ... of a pair of a slab's list (its own sphere ids; analytical components and triangles are numbered alike on every slab)
inline GlobalPair global_pair(const SlabIds& b, uint32_t la, uint32_t lb, uint8_t type) {
    return global_pair(b.sphereGid[la], type == DEME_SPHERE_SPHERE_CONTACT ? b.sphereGid[lb] : lb, type);
}
// a slab's list in its own ids (empty vectors: an empty list)
int slab_contacts(const SlabRef& r, std::vector<uint32_t>& a, std::vector<uint32_t>& b, std::vector<uint8_t>& t) {
    DemeCounts cnt{};
    if (int rc = deme_get_counts(r.c, &cnt))
        return rc;
    const size_t n = (size_t)cnt.nContacts;
    a.resize(n), b.resize(n), t.resize(n);
    return n ? deme_download_contacts(r.c, a.data(), b.data(), t.data(), nullptr, n) : DEME_OK;
}
}  // namespace

static int multi_contact_rows(deme_multi* m, std::vector<MultiRow>& rows) {
    rows.clear();
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            std::vector<uint32_t> a, b;
            std::vector<uint8_t> t;
            SlabIds ids;
            if (int rc = slab_contacts(r, a, b, t))
                return rc;
            if (int rc = slab_ids(m, r, IDS_SPHERE | IDS_SPHERE_OWNER, ids))
                return rc;
            for (size_t i = 0; i < t.size(); i++) {
                const GlobalPair gp = global_pair(ids, a[i], b[i], t[i]);
                if (ids.sphereOwner[gp.flipped ? b[i] : a[i]] >= r.s->geo.nOwn)
                    continue;  // the neighbour that owns that clump reports the pair
                rows.push_back({gp.key, r.no, (uint32_t)i, t[i], (uint8_t)gp.flipped});
            }
            return DEME_OK;
        }))
        return rc;
    std::sort(rows.begin(), rows.end(), [](const MultiRow& x, const MultiRow& y) { return x.key < y.key; });
    return DEME_OK;
}
static int multi_rows_cached(deme_multi* m) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (m->rowsAtStep == m->nSteps && m->rowsValid)
        return DEME_OK;
    if (int rc = deme_multi_sync(m))
        return rc;
    if (int rc = multi_contact_rows(m, m->rows))
        return rc;
    m->rowsAtStep = m->nSteps, m->rowsValid = true;
    return DEME_OK;
}
int deme_multi_num_contacts(deme_multi* m, size_t* n) {
    if (!n)
        return DEME_ERR_INVALID;
    if (int rc = multi_rows_cached(m))
        return rc;
    *n = m->rows.size();
    return DEME_OK;
}

int deme_multi_download_contacts(deme_multi* m, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap) {
    if (int rc = multi_rows_cached(m))
        return rc;
    if (cap < m->rows.size())
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", m->rows.size());
    for (size_t i = 0; i < m->rows.size(); i++) {
        const MultiRow& r = m->rows[i];
        if (idA)
            idA[i] = (uint32_t)(r.key >> 34);
        if (idB)
            idB[i] = (uint32_t)(r.key & 0x7FFFFFFFull);
        if (type)
            type[i] = r.type;
    }
    return DEME_OK;
}

int deme_multi_download_contact_wildcard(deme_multi* m, uint32_t w, float* out, size_t cap) {
    if (int rc = multi_rows_cached(m))
        return rc;
    if (m->rows.empty())
        return DEME_OK;  // (an empty list: nothing to write, whatever `out` is)
    if (!out)
        return mfail(m, DEME_ERR_INVALID, "deme_multi_download_contact_wildcard: null buffer for %zu rows", m->rows.size());
    if (cap < m->rows.size())
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", m->rows.size());
    std::vector<std::vector<float>> col(m->plan->nSlabs);
    std::vector<uint32_t> flipMask(m->plan->nSlabs, 0);
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            col[r.no].resize(std::max<size_t>(r.c->nContacts, 1));
            flipMask[r.no] = r.s->geo.flipMask;
            return r.c->nContacts ? deme_download_contact_wildcard(r.c, w, col[r.no].data(), r.c->nContacts) : DEME_OK;
        }))
        return rc;
    for (size_t i = 0; i < m->rows.size(); i++) {
        const MultiRow& r = m->rows[i];
        const float v = col[r.slab][r.row];
        out[i] = (r.flipped && ((flipMask[r.slab] >> w) & 1u)) ? -v : v;
    }
    return DEME_OK;
}

// writing a per-contact wildcard of the merged list: every slab's copy of a pair takes the caller's value (a pair across a cut has
// one row on each side), with the sign of the slab's own pair order for B -> A vector wildcards.  Rows of a slab that name no pair
// of the merged list (none: every listed pair involves an own clump of some slab) keep what they hold.
int deme_multi_upload_contact_wildcard(deme_multi* m, uint32_t w, const float* in, size_t n) {
    if (int rc = multi_rows_cached(m))
        return rc;
    if (m->rows.empty() && n == 0)
        return DEME_OK;
    if (!in)
        return mfail(m, DEME_ERR_INVALID, "deme_multi_upload_contact_wildcard: null column for %zu rows", m->rows.size());
    if (n != m->rows.size())
        return mfail(m, DEME_ERR_INVALID, "contact wildcard column of %zu values for a merged list of %zu pairs", n, m->rows.size());
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        std::vector<uint32_t> a, b;
        std::vector<uint8_t> t;
        SlabIds ids;
        if (int rc = slab_contacts(r, a, b, t))
            return rc;
        const size_t nc = t.size();
        if (!nc)
            return DEME_OK;
        std::vector<float> col(nc);
        if (int rc = deme_download_contact_wildcard(r.c, w, col.data(), nc))
            return rc;
        if (int rc = slab_ids(m, r, IDS_SPHERE, ids))
            return rc;
        for (size_t i = 0; i < nc; i++) {
            const GlobalPair gp = global_pair(ids, a[i], b[i], t[i]);
            auto it = std::lower_bound(m->rows.begin(), m->rows.end(), gp.key, [](const MultiRow& x, uint64_t k) { return x.key < k; });
            if (it == m->rows.end() || it->key != gp.key)
                continue;
            const float v = in[it - m->rows.begin()];
            col[i] = (gp.flipped && ((r.s->geo.flipMask >> w) & 1u)) ? -v : v;
        }
        return deme_upload_contact_wildcard(r.c, w, col.data(), nc);
    });
}

// ---- a saved list into a decomposed run (restart) and the marked (persistent) pairs, in GLOBAL ids ------------------------------------
// A pair goes to every slab that holds both of its geometries and owns at least one of them, in the slab's own ids, smaller sphere
// first, B -> A vector wildcards (the build's flipMask) with the slab's sign.
namespace {
struct SlabSpheres : SlabIds {
    std::vector<uint32_t> inv;  // global sphere id -> the slab's, or ~0
};
int slab_spheres(deme_multi* m, const SlabRef& r, SlabSpheres& b) {
    if (int rc = slab_ids(m, r, IDS_SPHERE | IDS_SPHERE_OWNER, b))
        return rc;
    b.inv.assign(m->plan->nSpheresGlobal, 0xFFFFFFFFu);
    for (uint32_t i = 0; i < r.c->nSpheres; i++)
        if (b.sphereGid[i] < b.inv.size())
            b.inv[b.sphereGid[i]] = i;
    return DEME_OK;
}
// the slab's form of a global pair; false: the slab does not hold it
inline bool slab_pair(const SlabSpheres& b, const HaloSlab& s, uint32_t gA, uint32_t gB, uint8_t type, uint32_t& la, uint32_t& lb, bool& flipped) {
    flipped = false;
    if (gA >= b.inv.size() || (la = b.inv[gA]) == 0xFFFFFFFFu)
        return false;
    if (type != DEME_SPHERE_SPHERE_CONTACT) {
        lb = gB;  // (analytical components and triangles are numbered alike on every slab)
        return b.sphereOwner[la] < s.geo.nOwn;
    }
    if (gB >= b.inv.size() || (lb = b.inv[gB]) == 0xFFFFFFFFu)
        return false;
    if (b.sphereOwner[la] >= s.geo.nOwn && b.sphereOwner[lb] >= s.geo.nOwn)
        return false;  // two ghosts: their owners' pair
    if (la > lb)
        std::swap(la, lb), flipped = true;
    return true;
}
}  // namespace

int deme_multi_seed_contacts(deme_multi* m, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, const float* wildcards, size_t n) {
    if (!m || !m->plan || (n && (!idA || !idB || !type)))
        return DEME_ERR_INVALID;
    if (int rc = deme_multi_sync(m))
        return rc;
    m->rowsValid = false;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        const uint32_t nW = r.c->hp.nContactWildcards;
        if (n && nW && !wildcards)
            return mfail(m, DEME_ERR_INVALID, "deme_multi_seed_contacts: the model keeps %u contact wildcards, none given", nW);
        SlabSpheres b;
        if (int rc = slab_spheres(m, r, b))
            return rc;
        std::vector<uint32_t> a, bb;
        std::vector<uint8_t> t;
        std::vector<float> w;
        for (size_t i = 0; i < n; i++) {
            uint32_t la, lb;
            bool flipped;
            const GlobalPair gp = global_pair(idA[i], idB[i], type[i]);  // (flipped: given larger id first, its vector wildcards are of that order)
            if (!slab_pair(b, *r.s, gp.a, gp.b, type[i], la, lb, flipped))
                continue;
            a.push_back(la), bb.push_back(lb), t.push_back(type[i]);
            for (uint32_t k = 0; k < nW; k++) {
                const float v = wildcards[i * nW + k];
                w.push_back(((flipped != gp.flipped) && ((r.s->geo.flipMask >> k) & 1u)) ? -v : v);
            }
        }
        return deme_seed_contacts(r.c, a.data(), bb.data(), t.data(), nW ? w.data() : nullptr, a.size());
    });
}

// the marked pairs of every slab, once each, in global ids (sphere-sphere pairs smaller id first), ascending
static int multi_persistent(deme_multi* m, std::vector<std::array<uint32_t, 3>>& out) {
    out.clear();
    if (int rc = deme_multi_sync(m))
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            size_t nP = 0;
            if (int rc = deme_num_persistent_contacts(r.c, &nP))
                return rc;
            if (!nP)
                return DEME_OK;
            std::vector<uint32_t> a(nP), b(nP);
            std::vector<uint8_t> t(nP);
            SlabIds ids;
            if (int rc = deme_download_persistent_contacts(r.c, a.data(), b.data(), t.data(), nP))
                return rc;
            if (int rc = slab_ids(m, r, IDS_SPHERE, ids))
                return rc;
            for (size_t i = 0; i < nP; i++) {
                const GlobalPair gp = global_pair(ids, a[i], b[i], t[i]);
                out.push_back({gp.a, gp.b, (uint32_t)t[i]});
            }
            return DEME_OK;
        }))
        return rc;
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return DEME_OK;
}
int deme_multi_num_persistent_contacts(deme_multi* m, size_t* n) {
    if (!m || !m->plan || !n)
        return DEME_ERR_INVALID;
    std::vector<std::array<uint32_t, 3>> v;
    if (int rc = multi_persistent(m, v))
        return rc;
    *n = v.size();
    return DEME_OK;
}
int deme_multi_download_persistent_contacts(deme_multi* m, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    std::vector<std::array<uint32_t, 3>> v;
    if (int rc = multi_persistent(m, v))
        return rc;
    if (cap < v.size())
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", v.size());
    for (size_t i = 0; i < v.size(); i++) {
        if (idA)
            idA[i] = v[i][0];
        if (idB)
            idB[i] = v[i][1];
        if (type)
            type[i] = (uint8_t)v[i][2];
    }
    return DEME_OK;
}
int deme_multi_upload_persistent_contacts(deme_multi* m, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, size_t n) {
    if (!m || !m->plan || (n && (!idA || !idB || !type)))
        return DEME_ERR_INVALID;
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        SlabSpheres b;
        if (int rc = slab_spheres(m, r, b))
            return rc;
        std::vector<uint32_t> a, bb;
        std::vector<uint8_t> t;
        for (size_t i = 0; i < n; i++) {
            uint32_t la, lb;
            bool flipped;
            const GlobalPair gp = global_pair(idA[i], idB[i], type[i]);
            if (slab_pair(b, *r.s, gp.a, gp.b, type[i], la, lb, flipped))
                a.push_back(la), bb.push_back(lb), t.push_back(type[i]);
        }
        return deme_upload_persistent_contacts(r.c, a.data(), bb.data(), t.data(), a.size());
    });
}
// deme_mark_persistent_contacts on every slab (the qualification is by families: the same rule everywhere)
int deme_multi_mark_persistent_contacts(deme_multi* m, int mode, uint32_t N1, uint32_t N2, int mark) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int { return deme_mark_persistent_contacts(r.c, mode, N1, N2, mark); });
}

int deme_multi_download_contact_records(deme_multi* m, float* force, float* torqueOnly, float* cpA, float* cpB, size_t cap) {
    if (int rc = multi_rows_cached(m))
        return rc;
    if (cap < m->rows.size())
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", m->rows.size());
    std::vector<std::vector<float>> f(m->plan->nSlabs), t(m->plan->nSlabs), a(m->plan->nSlabs), b(m->plan->nSlabs);
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            const size_t s = r.no, n = std::max<size_t>(r.c->nContacts, 1);
            f[s].resize(3 * n), t[s].resize(3 * n), a[s].resize(3 * n), b[s].resize(3 * n);
            return r.c->nContacts ? deme_download_contact_records(r.c, f[s].data(), t[s].data(), a[s].data(), b[s].data(), r.c->nContacts) : DEME_OK;
        }))
        return rc;
    for (size_t i = 0; i < m->rows.size(); i++) {
        const MultiRow& r = m->rows[i];
        const float sgn = r.flipped ? -1.f : 1.f;  // (the recorded force acts on A: the other body takes the opposite one)
        for (int k = 0; k < 3; k++) {
            if (force)
                force[3 * i + k] = sgn * f[r.slab][3 * (size_t)r.row + k];
            if (torqueOnly)
                torqueOnly[3 * i + k] = sgn * t[r.slab][3 * (size_t)r.row + k];
            if (cpA)
                cpA[3 * i + k] = (r.flipped ? b : a)[r.slab][3 * (size_t)r.row + k];
            if (cpB)
                cpB[3 * i + k] = (r.flipped ? a : b)[r.slab][3 * (size_t)r.row + k];
        }
    }
    return DEME_OK;
}

// ---- the contacts and the state of a few owners of a decomposed run, selected on every slab's device (deme_query.h) -----------------
// Every slab selects from its own list with the rule of multi_contact_rows (k_query_select<true> through the query_mark / _select /
// _fetch of deme_hip.hip: global ids from the books the migration keeps on the device) and hands over a count and its hit rows;
// the host sorts the hits of all slabs by the merged key (a pair is reported once, so keys are unique).  The cached merged rows
// are neither used nor invalidated.
namespace {
inline SlabBooksDev slab_books_dev(const HaloSlab& s, uint32_t nOwnersGlobal) {
    SlabBooksDev bk{};
    bk.sphereGid = (const uint32_t*)s.geo.sphereGid, bk.ownerGid = (const uint32_t*)s.geo.ownerGid;
    bk.nOwn = s.geo.nOwn, bk.nOwnersGlobal = nOwnersGlobal;
    return bk;
}
// one slab's owners of a question: their records gathered into the context's scratch (at most ids.size() of them), the count in nHit
int slab_query_state(const SlabRef& r, uint32_t nOwnersGlobal, size_t nIds, uint32_t& nHit) {
    deme_ctx* c = r.c;
    nHit = 0;
    if (!c->nOwners)
        return DEME_OK;
    if (ensure(c, c->qState, nIds * sizeof(OwnerRec)))
        return c->lastStatus;
    const SlabBooksDev bk = slab_books_dev(*r.s, nOwnersGlobal);
    HIPCK(hipMemsetAsync(c->qCtr.p, 0, 4, c->stream));
    // (takeReplicated = r.first: the kernel applies slab_reports to the slots it visits)
    hipLaunchKernelGGL(k_query_owner_state, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->nOwners, c->owners.as<OwnerRec>(),
                       (const uint32_t*)nullptr, c->dp.o2e, bk, c->nOwnerClumps, r.first ? 1u : 0u, c->qMark.as<uint8_t>(),
                       c->qState.as<OwnerRec>(), (uint32_t)std::min<size_t>(c->qState.bytes / sizeof(OwnerRec), 0xFFFFFFFFu),
                       c->qCtr.as<uint32_t>());
    HIPCK(hipMemcpyAsync(&nHit, c->qCtr.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
int slab_query_fetch_state(deme_ctx* c, uint32_t nHit, OwnerRec* h) {
    HIPCK(hipMemcpyAsync(h, c->qState.p, (size_t)nHit * sizeof(OwnerRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

int deme_multi_query_owner_contacts(deme_multi* m, const uint32_t* ownerIds, size_t nOwners, int withRecords, uint32_t* idA, uint32_t* idB,
                                    uint8_t* type, uint32_t* ownerA, uint32_t* ownerB, uint8_t* side, float* force, float* torqueOnly,
                                    float* cpA, float* cpB, size_t cap, size_t* nOut) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const uint32_t nOG = m->plan->nOwnersGlobal;
    char msg[320];
    if (int rc = owner_ids_refused(msg, "deme_multi_query_owner_contacts", nOut, "nOut", ownerIds, nOwners, nOG))
        return mfail(m, rc, "%s", msg);
    if (int rc = deme_multi_sync(m))
        return rc;
    if (withRecords)
        if (int rc = multi_slabs(m, slab_records_refused))
            return rc;
    std::vector<uint32_t> ids(ownerIds, ownerIds + nOwners);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<uint32_t> nHit(m->plan->nSlabs, 0);
    size_t total = 0;
    if (!ids.empty())
        if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
                deme_ctx* c = r.c;
                if (!r.s->geo.set)
                    return mfail(m, DEME_ERR_INVALID, "deme_multi_query_owner_contacts: a slab has no books (deme_halo_group_set_slab / _build)");
                uint32_t passes = 0;
                if (c->haveList && c->nContacts) {
                    const SlabBooksDev bk = slab_books_dev(*r.s, nOG);
                    if (int rc = query_mark(c, ids, std::max<size_t>(nOG, 1)))
                        return rc;
                    if (int rc = query_select(c, &bk, "deme_multi_query_owner_contacts", withRecords, nHit[r.no], passes))
                        return rc;
                }
                m->qHostBytes += 4ull * passes;  // (a slab with an empty list is not asked)
                total += nHit[r.no];
                return DEME_OK;
            }))
            return rc;
    *nOut = total;
    if (cap < total)
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", total);
    if (!total)
        return DEME_OK;
    std::vector<QueryHit> h(total);
    std::vector<float> r(withRecords ? total * 12 : 0);
    std::vector<const deme_ctx*> ctxOf(total);
    size_t at = 0;
    if (int rc = multi_slabs(m, [&](const SlabRef& sl) -> int {
            const uint32_t n = nHit[sl.no];
            if (!n)
                return DEME_OK;
            if (int rc = query_fetch(sl.c, n, withRecords, h.data() + at, withRecords ? r.data() + 12 * at : nullptr))
                return rc;
            std::fill_n(ctxOf.begin() + at, n, sl.c);
            at += n;
            return DEME_OK;
        }))
        return rc;
    m->qHostBytes += (uint64_t)total * (sizeof(QueryHit) + (withRecords ? 48 : 0));
    query_emit(h, r, true, [&](uint32_t hit) { return ctxOf[hit]; }, QueryRows{idA, idB, type, ownerA, ownerB, side, {force, torqueOnly, cpA, cpB}});
    return DEME_OK;
}

int deme_multi_query_host_bytes(const deme_multi* m, uint64_t* bytes) {
    if (!m || !bytes)
        return DEME_ERR_INVALID;
    *bytes = m->qHostBytes;
    return DEME_OK;
}

int deme_multi_query_owner_state(deme_multi* m, const uint32_t* globalIds, size_t n, DemeOwnerState* out) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const uint32_t nOG = m->plan->nOwnersGlobal;
    char msg[320];
    if (int rc = owner_ids_refused(msg, "deme_multi_query_owner_state", out, "state", globalIds, n, nOG, out,
                                   "need the reduction a full download launches (deme_multi_download_state)"))
        return mfail(m, rc, "%s", msg);
    if (!n)
        return DEME_OK;
    if (int rc = deme_multi_sync(m))
        return rc;
    // the rows of `out` every distinct id fills: (id, row) sorted by id
    std::vector<std::pair<uint32_t, uint32_t>> rowsOf(n);
    for (size_t i = 0; i < n; i++)
        rowsOf[i] = {globalIds[i], (uint32_t)i};
    std::sort(rowsOf.begin(), rowsOf.end());
    std::vector<uint32_t> ids;
    for (auto& pr : rowsOf)
        if (ids.empty() || ids.back() != pr.first)
            ids.push_back(pr.first);
    size_t found = 0;
    std::vector<OwnerRec> h;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            deme_ctx* c = r.c;
            if (!r.s->geo.set)
                return mfail(m, DEME_ERR_INVALID, "deme_multi_query_owner_state: a slab has no books (deme_halo_group_set_slab / _build)");
            uint32_t nHit = 0;
            if (int rc = query_mark(c, ids, std::max<size_t>(nOG, 1)))
                return rc;
            if (int rc = slab_query_state(r, nOG, ids.size(), nHit))
                return rc;
            m->qHostBytes += 4;
            if (nHit > ids.size())
                return mfail(m, DEME_ERR_INVALID, "deme_multi_query_owner_state: a slab holds %u owners for %zu ids", nHit, ids.size());
            if (!nHit)
                return DEME_OK;
            h.resize(nHit);
            if (int rc = slab_query_fetch_state(c, nHit, h.data()))
                return rc;
            m->qHostBytes += (uint64_t)nHit * sizeof(OwnerRec);
            for (uint32_t i = 0; i < nHit; i++) {
                uint32_t gid;
                memcpy(&gid, &h[i].margin, 4);
                auto it = std::lower_bound(rowsOf.begin(), rowsOf.end(), std::make_pair(gid, 0u));
                for (; it != rowsOf.end() && it->first == gid; ++it)
                    owner_state_row(out, it->second, h[i]);
                found++;
            }
            return DEME_OK;
        }))
        return rc;
    if (found != ids.size())
        return mfail(m, DEME_ERR_INVALID, "deme_multi_query_owner_state: %zu of %zu owners were found on the slabs", found, ids.size());
    return DEME_OK;
}

// deme_scatter_owner_state by GLOBAL owner id.  Every slab receives the asked ids in ascending order with their records and one
// thread per owner slot searches its global id among them (k_scatter_owner_state): the clump in the slab that owns it, its ghost
// copies in the neighbours and the replicated owners on every slab all take the value, as group_state_io writes them on upload.
int deme_multi_scatter_owner_state(deme_multi* m, const uint32_t* globalIds, size_t n, const DemeOwnerState* in) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    char msg[320];
    std::vector<std::pair<uint32_t, uint32_t>> sorted;
    if (int rc = owner_ids_refused(msg, "deme_multi_scatter_owner_state", in, "state", globalIds, n, m->plan->nOwnersGlobal, in,
                                   "columns are not written by owner id (deme_upload_owner_state hands the accumulators to the caller)", true, &sorted))
        return mfail(m, rc, "%s", msg);
    const uint32_t mask = owner_state_mask(in);
    if (!n || !mask)
        return DEME_OK;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            return r.s->geo.set ? DEME_OK : mfail(m, DEME_ERR_INVALID, "deme_multi_scatter_owner_state: a slab has no books (deme_halo_group_set_slab / _build)");
        }))
        return rc;
    if (int rc = deme_multi_sync(m))
        return rc;
    std::vector<uint32_t> ids(n);
    std::vector<OwnerRec> patch(n);
    for (size_t i = 0; i < n; i++) {
        ids[i] = sorted[i].first;
        patch[i] = owner_state_patch(in, sorted[i].second);
    }
    m->rowsValid = false;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        if (int rc = check_ready(r.c))
            return rc;
        if (int rc = launch_owner_scatter(r.c, in, ids, patch, mask, true, (const uint32_t*)r.s->geo.ownerGid))
            return rc;
        m->qHostBytes += (uint64_t)n * (4 + sizeof(OwnerRec));
        return DEME_OK;
    });
}

// accelerations a script adds for the next step (deme_add_owner_acc), by GLOBAL owner id: a clump's go to the slab that owns it, a
// replicated owner's (walls, meshes: the same on every slab) to every slab
int deme_multi_add_owner_acc(deme_multi* m, uint32_t owner, uint32_t n, const float* acc, const float* angAcc) {
    if (!m || !m->plan || (!acc && !angAcc))
        return DEME_ERR_INVALID;
    if ((uint64_t)owner + n > m->plan->nOwnersGlobal)
        return mfail(m, DEME_ERR_INVALID, "deme_multi_add_owner_acc: owners [%u, %u) out of range", owner, owner + n);
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        deme_ctx* c = r.c;
        SlabIds ids;
        if (int rc = slab_ids(m, r, IDS_OWNER, ids))
            return rc;
        const std::vector<uint32_t>& gid = ids.ownerGid;
        auto wanted = [&](uint32_t i) { return slab_takes(r, i) && gid[i] >= owner && gid[i] < owner + n; };  // (ghosts are their owner slab's)
        for (uint32_t i = 0; i < c->nOwners;) {  // runs of slots whose global ids run along: one call (one copy, one wait) per run
            if (!wanted(i)) {
                i++;
                continue;
            }
            uint32_t j = i + 1;
            while (j < c->nOwners && wanted(j) && gid[j] == gid[j - 1] + 1u)
                j++;
            const uint32_t k = gid[i] - owner;
            if (int rc = deme_add_owner_acc(c, i, j - i, acc ? acc + 3 * (size_t)k : nullptr, angAcc ? angAcc + 3 * (size_t)k : nullptr))
                return rc;
            i = j;
        }
        return DEME_OK;
    });
}

// a user model's wildcard arrays by GLOBAL id (kind 0: per owner, 1: per sphere): a row comes from the slab that owns the clump (a
// replicated owner's from the first slab), and goes to every copy.  Triangles' and analytical components' arrays (kinds 2, 3) are
// replicated geometry: written to every slab, read back from the FIRST slab -- with every other slab's copy compared against it: a
// model that writes them from its contacts keeps a part per slab, and a download of such an array is refused loudly (the parts are
// reached through deme_multi_slab_ctx).
static int multi_wc_io(deme_multi* m, uint32_t kind, uint32_t index, float* glob, size_t n, bool down) {
    if (!m || !m->plan || !glob || kind > 3 || index >= 8)
        return DEME_ERR_INVALID;
    const size_t want = kind == 0 ? m->plan->nOwnersGlobal : kind == 1 ? m->plan->nSpheresGlobal : 0;
    if (kind < 2 && n != want)
        return mfail(m, DEME_ERR_INVALID, "wildcard array of kind %u of a decomposed run holds %zu values, %zu given", kind, want, n);
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        deme_ctx* c = r.c;
        if (kind >= 2) {  // replicated geometry: written everywhere; read from the first slab, and the others must agree with it
            if (down && !r.first) {
                // A model that WRITES these arrays from its contacts (Models.h:345-360: triWildcards, analWildcards) leaves a
                // different part in every slab -- a triangle's contacts are evaluated by the slabs that own the spheres.  There is no
                // rule that merges parts of an arbitrary user quantity (a sum? a maximum? the last writer?), so a run whose slabs
                // disagree says so instead of handing back one slab's part as if it were the whole.
                std::vector<float> other(std::max<size_t>(n, 1));
                if (int rc = deme_download_wildcard_array(c, kind, index, other.data(), n))
                    return rc;
                if (n && memcmp(other.data(), glob, n * sizeof(float)) != 0)
                    return mfail(m, DEME_ERR_INVALID,
                                 "%s wildcard array %u differs between the slabs of this decomposed run: the force model writes it, and each slab "
                                 "holds the part of the contacts it evaluated (read the parts through deme_multi_slab_ctx + "
                                 "deme_download_wildcard_array and combine them as the quantity asks)",
                                 kind == 2 ? "triangle" : "analytical-geometry", index);
                return DEME_OK;
            }
            return down ? deme_download_wildcard_array(c, kind, index, glob, n) : deme_upload_wildcard_array(c, kind, index, glob, n);
        }
        const size_t nLoc = kind == 0 ? c->nOwners : c->nSpheres;
        SlabIds ids;
        if (int rc = slab_ids(m, r, kind == 0 ? IDS_OWNER : down ? IDS_SPHERE | IDS_SPHERE_OWNER : IDS_SPHERE, ids))
            return rc;
        const std::vector<uint32_t>& gid = kind == 0 ? ids.ownerGid : ids.sphereGid;
        std::vector<float> loc(std::max<size_t>(nLoc, 1));
        for (size_t i = 0; i < nLoc; i++)
            if (gid[i] >= want)
                return mfail(m, DEME_ERR_INVALID, "wildcard array by global id: slab %zu slot %zu names id %u of %zu", (size_t)r.no, i, gid[i], want);
        if (!down) {
            for (size_t i = 0; i < nLoc; i++)
                loc[i] = glob[gid[i]];
            return deme_upload_wildcard_array(c, kind, index, loc.data(), nLoc);
        }
        if (int rc = deme_download_wildcard_array(c, kind, index, loc.data(), nLoc))
            return rc;
        for (size_t i = 0; i < nLoc; i++)
            if (slab_reports(r, kind == 0 ? (uint32_t)i : ids.sphereOwner[i]))
                glob[gid[i]] = loc[i];
        return DEME_OK;
    });
}
int deme_multi_download_wildcard_array(deme_multi* m, uint32_t kind, uint32_t index, float* out, size_t cap) {
    return multi_wc_io(m, kind, index, out, cap, true);
}
int deme_multi_upload_wildcard_array(deme_multi* m, uint32_t kind, uint32_t index, const float* in, size_t n) {
    return multi_wc_io(m, kind, index, const_cast<float*>(in), n, false);
}

// deme_inspect_values of a decomposed run: one value per sphere (codes up to DEME_INSPECT_CLUMP_MAX_ABSV) or per owner, by GLOBAL id;
// a clump's rows come from the slab that owns it, a replicated owner's from the first slab
int deme_multi_inspect_values(deme_multi* m, uint32_t q, float* out, size_t cap) {
    if (!m || !m->plan || !out)
        return DEME_ERR_INVALID;
    const bool perSphere = q <= DEME_INSPECT_CLUMP_MAX_ABSV;
    const size_t want = perSphere ? m->plan->nSpheresGlobal : m->plan->nOwnersGlobal;
    if (cap < want)
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", want);
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        const size_t nLoc = perSphere ? r.c->nSpheres : r.c->nOwners;
        std::vector<float> loc(std::max<size_t>(nLoc, 1));
        if (int rc = deme_inspect_values(r.c, q, loc.data(), nLoc))
            return rc;
        SlabIds ids;
        if (int rc = slab_ids(m, r, perSphere ? IDS_SPHERE | IDS_SPHERE_OWNER : IDS_OWNER, ids))
            return rc;
        for (size_t i = 0; i < nLoc; i++) {
            const uint32_t gid = perSphere ? ids.sphereGid[i] : ids.ownerGid[i];
            if (slab_reports(r, perSphere ? ids.sphereOwner[i] : (uint32_t)i) && gid < want)
                out[gid] = loc[i];
        }
        return DEME_OK;
    });
}

// ---- contact inspectors of a decomposed run (deme_contact_inspect.h) ------------------------------------------------------------------
// Every slab runs the single context's passes over its own list; its mask holds its own clumps only (a ghost copy carries the ghost
// bit), so a contact across a cut gives one side on each of its two slabs.  The host adds the slabs' answers in slab order.
namespace {
// the region of a slab context for a region string: compiled on first use, then found by its text; blank: -1
int slab_region(deme_ctx* c, const char* code, int* id) {
    const std::string src = code ? code : "";
    *id = -1;
    if (src.find_first_not_of(" \t\r\n") == std::string::npos)
        return DEME_OK;
    auto it = c->regionBySource.find(src);
    if (it == c->regionBySource.end()) {
        int rid = -1;
        if (int rc = deme_compile_region(c, src.c_str(), &rid))
            return rc;
        it = c->regionBySource.emplace(src, rid).first;
    }
    *id = it->second;
    return DEME_OK;
}
// A run that evaluates every cross-cut contact once cannot sum the sides of its pairs.  (Nothing sets pairsOnce on a deme_multi's
// groups today, so the branch is not reached.)
int multi_pairs_once_refused(deme_multi* m, const char* who) {
    for (auto* g : m->groups)
        if (g->pairsOnce)
            return mfail(m, DEME_ERR_INVALID, "%s: the run evaluates every cross-cut contact once (deme_halo_group_set_cross_contacts): the slab that "
                         "does not evaluate a pair holds no record of it, so its side of the pair cannot be summed", who);
    return DEME_OK;
}
// what both calls refuse before any slab is asked, and the slabs' regions (in slab order)
int multi_contact_inspect_begin(deme_multi* m, const char* who, const void* out, const char* regionCode, float thr, std::vector<int>& regions) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (!out)
        return mfail(m, DEME_ERR_INVALID, "%s: null output", who);
    char msg[320];
    if (threshold_refused(msg, who, thr))
        return mfail(m, DEME_ERR_INVALID, "%s", msg);
    if (int rc = multi_pairs_once_refused(m, who))
        return rc;
    if (int rc = deme_multi_sync(m))
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (!r.s->geo.set)
                return mfail(m, DEME_ERR_INVALID, "%s: a slab has no books (deme_halo_group_set_slab / _build)", who);
            return slab_records_refused(r);
        }))
        return rc;
    regions.clear();
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        int rid = -1;
        if (int rc = slab_region(r.c, regionCode, &rid))
            return rc;
        regions.push_back(rid);
        return DEME_OK;
    });
}
// one slab's counted sides per owner slot (left in ciCounts by contact_inspect_launch) added at the global ids of h
int slab_contact_counts(deme_ctx* c, const HaloSlab& s, uint32_t nOG, std::vector<uint32_t>& h) {
    if (ensure(c, c->ciOut, std::max<size_t>(nOG, 1) * 4))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->ciOut.p, 0, (size_t)nOG * 4, c->stream));
    if (c->nOwners)
        hipLaunchKernelGGL(k_contact_counts_out, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->nOwners, c->ciCounts.as<uint32_t>(),
                           c->dp.o2e, (const uint32_t*)s.geo.ownerGid, c->ciOut.as<uint32_t>(), nOG);
    h.resize(nOG);
    HIPCK(hipMemcpyAsync(h.data(), c->ciOut.p, (size_t)nOG * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
int slab_contact_sums(deme_ctx* c, int region, float thr, DemeContactSums* h) {
    ContactSums* res = nullptr;
    if (int rc = contact_inspect_launch(c, region, thr, false, &res))
        return rc;
    HIPCK(hipMemcpyAsync(h, res, sizeof *h, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

int deme_multi_inspect_contacts(deme_multi* m, const char* regionCode, float thr, DemeContactSums* out) {
    std::vector<int> regions;
    if (int rc = multi_contact_inspect_begin(m, "deme_multi_inspect_contacts", out, regionCode, thr, regions))
        return rc;
    DemeContactSums sum{};
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            DemeContactSums h{};
            if (int rc = slab_contact_sums(r.c, regions[r.no], thr, &h))
                return rc;
            m->qHostBytes += sizeof h;
            for (int j = 0; j < 9; j++)
                sum.virial[j] += h.virial[j];
            sum.sides += h.sides, sum.clumps += h.clumps;
            return DEME_OK;
        }))
        return rc;
    *out = sum;
    return DEME_OK;
}

int deme_multi_inspect_contact_counts(deme_multi* m, const char* regionCode, float thr, uint32_t* perOwnerGlobal, size_t cap) {
    std::vector<int> regions;
    if (m && m->plan && perOwnerGlobal && cap < m->plan->nOwnersGlobal)
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %zu", (size_t)m->plan->nOwnersGlobal);
    if (int rc = multi_contact_inspect_begin(m, "deme_multi_inspect_contact_counts", perOwnerGlobal, regionCode, thr, regions))
        return rc;
    const uint32_t nOG = m->plan->nOwnersGlobal;
    std::vector<uint32_t> sum(nOG, 0u), h;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (int rc = contact_inspect_launch(r.c, regions[r.no], thr, true, nullptr))
                return rc;
            if (int rc = slab_contact_counts(r.c, *r.s, nOG, h))
                return rc;
            m->qHostBytes += 4ull * nOG;
            for (uint32_t i = 0; i < nOG; i++)
                sum[i] += h[i];
            return DEME_OK;
        }))
        return rc;
    if (nOG)
        memcpy(perOwnerGlobal, sum.data(), (size_t)nOG * 4);
    return DEME_OK;
}

// ---- contact loads per mesh triangle of a decomposed run (deme_tri_loads.h) -------------------------------------------------------------
// Triangles carry the same ids on every slab, and a row whose sphere belongs to a ghost copy is not counted: every sphere-triangle
// pair is counted by the one slab that owns the sphere's clump.  All slabs' passes are enqueued first, each on its device, then the
// host takes the asked range slab by slab and adds the arrays in slab order.  (The pairsOnce refusal mirrors the contact
// inspectors'.)
int deme_multi_inspect_tri_loads(deme_multi* m, float thr, uint32_t firstTri, uint32_t nTris, double* force, uint32_t* contacts) {
    const char* who = "deme_multi_inspect_tri_loads";
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const SlabRef head = multi_slab(m, 0);
    char msg[320];
    if (int rc = tri_loads_args_refused(msg, who, thr, firstTri, nTris, head.c ? head.c->nTri : 0u, force, contacts))
        return mfail(m, rc, "%s", msg);
    if (!nTris)
        return DEME_OK;
    if (int rc = multi_pairs_once_refused(m, who))
        return rc;
    if (int rc = deme_multi_sync(m))
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (slab_records_refused(r))
                return mfail(m, DEME_ERR_INVALID, "%s: %s", who, r.c->err.c_str());
            return DEME_OK;
        }))
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int { return tri_loads_launch(r.c, thr); }))
        return rc;
    std::vector<double> sumF(force ? (size_t)nTris * 3 : 0, 0.0), hf(sumF.size());
    std::vector<uint32_t> sumN(contacts ? nTris : 0, 0u), hn(sumN.size());
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (int rc = tri_loads_fetch(r.c, firstTri, nTris, force ? hf.data() : nullptr, contacts ? hn.data() : nullptr))
                return rc;
            m->qHostBytes += (uint64_t)nTris * ((force ? 24 : 0) + (contacts ? 4 : 0));
            for (size_t i = 0; i < sumF.size(); i++)
                sumF[i] += hf[i];
            for (size_t i = 0; i < sumN.size(); i++)
                sumN[i] += hn[i];
            return DEME_OK;
        }))
        return rc;
    if (force)
        memcpy(force, sumF.data(), sumF.size() * 8);
    if (contacts)
        memcpy(contacts, sumN.data(), sumN.size() * 4);
    return DEME_OK;
}

// ---- mesh wear of a decomposed run (deme_tri_wear.h) -------------------------------------------------------------------------------------
// Every slab samples its own list on its own device into its own accumulators; a pair is counted by the one slab that owns sphere
// A's clump (ghost rows are not counted).  A sample is all or nothing: the slabs are asked first, and if any slab's list is a seed
// -- the step after a migration -- no slab adds anything.  A read adds the slabs' arrays in slab order.
namespace {
bool multi_wear_enabled(deme_multi* m) {
    bool on = true;
    multi_slabs(m, [&](const SlabRef& r) -> int {
        on = on && r.c->twOn;
        return DEME_OK;
    });
    return on;
}
}  // namespace

int deme_multi_tri_wear_enable(deme_multi* m, int on) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (on)
        if (int rc = multi_pairs_once_refused(m, "deme_multi_tri_wear_enable"))
            return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int { return deme_tri_wear_enable(r.c, on); });
}

int deme_multi_tri_wear_reset(deme_multi* m) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    if (!multi_wear_enabled(m))
        return mfail(m, DEME_ERR_INVALID, "deme_multi_tri_wear_reset: mesh wear accumulation is not enabled (deme_multi_tri_wear_enable)");
    return multi_slabs(m, [&](const SlabRef& r) -> int { return deme_tri_wear_reset(r.c); });
}

int deme_multi_tri_wear_sample(deme_multi* m, float thr, double weight, int* sampled) {
    const char* who = "deme_multi_tri_wear_sample";
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    char msg[320];
    if (int rc = tri_wear_sample_refused(msg, who, multi_wear_enabled(m), thr, weight))
        return mfail(m, rc, "%s", msg);
    if (int rc = multi_pairs_once_refused(m, who))
        return rc;
    bool seed = false;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (!r.c->record)
                return mfail(m, DEME_ERR_INVALID, "%s: contact recording is off (deme_set_record_contacts)", who);
            seed = seed || tri_wear_list_unevaluated(r.c);
            return DEME_OK;
        }))
        return rc;
    if (sampled)
        *sampled = 0;
    if (seed)
        return DEME_OK;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int { return tri_wear_launch(r.c, thr, weight); }))
        return rc;
    if (sampled)
        *sampled = 1;
    return DEME_OK;
}

int deme_multi_tri_wear_read(deme_multi* m, uint32_t firstTri, uint32_t nTris, double* impulse, double* normalImpulse, double* slidingWork,
                             double* shearWork, uint64_t* rows, double* sampledTime) {
    const char* who = "deme_multi_tri_wear_read";
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const SlabRef head = multi_slab(m, 0);
    char msg[320];
    const bool any = impulse || normalImpulse || slidingWork || shearWork || rows || sampledTime;
    if (int rc = tri_wear_read_refused(msg, who, multi_wear_enabled(m), firstTri, nTris, head.c ? head.c->nTri : 0u, any))
        return mfail(m, rc, "%s", msg);
    if (int rc = multi_pairs_once_refused(m, who))
        return rc;
    if (nTris) {
        if (int rc = deme_multi_sync(m))
            return rc;
        void* dst[5] = {impulse, normalImpulse, slidingWork, shearWork, rows};
        const bool want[5] = {impulse != nullptr, normalImpulse != nullptr, slidingWork != nullptr, shearWork != nullptr, rows != nullptr};
        std::vector<char> h;
        std::vector<double> sum[4];
        std::vector<uint64_t> sumRows(rows ? nTris : 0, 0ull);
        for (int j = 0; j < 4; j++)
            sum[j].assign(want[j] ? WEAR_COL_BYTES[j] / 8 * nTris : 0, 0.0);
        if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
                if (int rc = tri_wear_fetch(r.c, firstTri, nTris, want, h))
                    return rc;
                m->qHostBytes += h.size();
                for (int j = 0; j < 4; j++) {
                    const double* col = (const double*)tri_wear_column(h, nTris, want, j);
                    for (size_t i = 0; i < sum[j].size(); i++)
                        sum[j][i] += col[i];
                }
                const uint64_t* col = (const uint64_t*)tri_wear_column(h, nTris, want, 4);
                for (size_t i = 0; i < sumRows.size(); i++)
                    sumRows[i] += col[i];
                return DEME_OK;
            }))
            return rc;
        for (int j = 0; j < 4; j++)
            if (want[j])
                memcpy(dst[j], sum[j].data(), sum[j].size() * 8);
        if (rows)
            memcpy(rows, sumRows.data(), sumRows.size() * 8);
    }
    if (sampledTime)
        *sampledTime = head.c ? head.c->twTime : 0.0;
    return DEME_OK;
}

// ---- per-cell sums on a grid of a decomposed run (deme_fields.h) ------------------------------------------------------------------------
// Every slab holds its clumps in the world frame and counts its own clumps only (ghost copies never count), so a clump, and every
// side it carries, is counted by one slab.  All slabs' passes are enqueued first, each on its device, then the host takes the asked
// columns slab by slab and adds them in slab order.  The refusals of the contact inspectors (pairsOnce; a slab whose list is a seed, as
// on the step after a migration) apply only when a contact column is asked.
int deme_multi_inspect_fields(deme_multi* m, const DemeFieldGrid* grid, float thr, const DemeFieldColumns* out) {
    const char* who = "deme_multi_inspect_fields";
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    char msg[320];
    if (int rc = fields_args_refused(msg, who, grid, thr, out))
        return mfail(m, rc, "%s", msg);
    const bool askOwner = fields_ask_owner(out), askContact = fields_ask_contact(out);
    if (askContact)
        if (int rc = multi_pairs_once_refused(m, who))
            return rc;
    if (int rc = deme_multi_sync(m))
        return rc;
    DemeFieldColumns perSlab = *out;  // (a slab with an empty list is not asked for its records: slab_records_refused)
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            perSlab.sides = r.c->nContacts ? out->sides : nullptr, perSlab.virial = r.c->nContacts ? out->virial : nullptr;
            return fields_ctx_refused(r.c, &perSlab);
        }))
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int { return fields_launch(r.c, grid, thr, askOwner, askContact); }))
        return rc;
    const size_t nC = (size_t)grid->n[0] * grid->n[1] * grid->n[2];
    FieldHost sum(out, nC), h(out, nC);
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (int rc = fields_fetch(r.c, nC, h))
                return rc;
            m->qHostBytes += h.bytes;
            sum.add(h);
            return DEME_OK;
        }))
        return rc;
    sum.hand_over(out);
    return DEME_OK;
}

// ---- connected components of the contact network of a decomposed run (deme_clusters.h) -------------------------------------------------
// A slab sees its own clumps and the ghost copies beside them, so it can link what touches inside its reach and nothing more: a
// cluster that crosses a cut is two (or more) local trees, each holding the ghost copy of the clump on the other side.  Every slab
// hands down, per local owner, the pair (global id, global id of its local root); the host unites every pair in one array
// union-find over the global ids -- the smaller root wins, as on the device -- and the label is the root.  A slab's table counts its
// OWN clumps only, so a clump is counted once; its rows are added into their final label in slab order, local roots ascending.
int deme_multi_inspect_clusters(deme_multi* m, float thr, DemeClusterSummary* summary, uint32_t* labels, size_t labelCap,
                                const DemeClusterColumns* table, size_t tableCap, size_t* nClusters) {
    const char* who = "deme_multi_inspect_clusters";
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const uint32_t nOG = m->plan->nOwnersGlobal;
    char msg[320];
    if (int rc = clusters_args_refused(msg, who, summary, labels, labelCap, nOG, table, nClusters, thr))
        return mfail(m, rc, "%s", msg);
    std::vector<int> regions;
    if (int rc = multi_contact_inspect_begin(m, who, m, nullptr, thr, regions))  // (pairsOnce; the wait; the slabs' books and records)
        return rc;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            if (r.c->haveList && r.c->nContacts >= ((uint64_t)1 << 31))
                return mfail(m, DEME_ERR_INVALID, "%s: a slab's list has %llu rows; the rows are indexed with 32 bits", who,
                             (unsigned long long)r.c->nContacts);
            return DEME_OK;
        }))
        return rc;
    const bool askTable = table || nClusters || summary;  // (the summary's sizes come from the merged table)
    const ClusterAsk ask{summary != nullptr, true, askTable, askTable};
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            deme_ctx* c = r.c;
            if (int rc = clusters_launch(c, thr, (const uint32_t*)r.s->geo.ownerGid, ask))
                return rc;
            if (!c->nOwners)
                return DEME_OK;
            if (ensure(c, c->clPairs, (size_t)c->nOwners * 8))
                return c->lastStatus;
            hipLaunchKernelGGL(k_cluster_pairs, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->nOwners, c->clLabel.as<uint32_t>(),
                               (const uint32_t*)r.s->geo.ownerGid, c->clPairs.as<uint2>());
            HIPCK(hipGetLastError());
            return DEME_OK;
        }))
        return rc;
    // the forest over the global ids
    std::vector<uint32_t> parent(nOG, 0xFFFFFFFFu);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) {
            parent[x] = parent[parent[x]];
            x = parent[x];
        }
        return x;
    };
    struct SlabRows {
        std::vector<uint32_t> rootGid;  // of every row of the slab's table
        ClusterRows rows{true, true, true, true, 0};
    };
    std::vector<SlabRows> perSlab;
    uint64_t edges = 0;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            deme_ctx* c = r.c;
            ClusterCtl ctl{};
            DemeClusterSummary sum{};
            if (int rc = clusters_fetch_head(c, ask.summary, &ctl, &sum))
                return rc;
            m->qHostBytes += sizeof ctl + (ask.summary ? sizeof sum : 0);
            edges += sum.edges;
            const size_t nO = c->nOwners, rows = ask.table ? (size_t)ctl.nRows : 0;
            std::vector<uint2> pairs(nO);
            perSlab.emplace_back();
            SlabRows& s = perSlab.back();
            s.rows = ClusterRows(true, true, true, true, rows);
            if (nO)
                HIPCK(hipMemcpyAsync(pairs.data(), c->clPairs.p, nO * 8, hipMemcpyDeviceToHost, c->stream));
            if (int rc = clusters_fetch_rows(c, s.rows))
                return rc;
            HIPCK(hipStreamSynchronize(c->stream));
            m->qHostBytes += 8ull * nO + s.rows.bytes;
            for (const uint2& p : pairs) {
                if (p.x >= nOG || p.y >= nOG)  // (no vertex)
                    continue;
                for (uint32_t g : {p.x, p.y})
                    if (parent[g] == 0xFFFFFFFFu)
                        parent[g] = g;
                const uint32_t a = find(p.x), b = find(p.y);
                if (a != b)
                    parent[std::max(a, b)] = std::min(a, b);
            }
            s.rootGid.resize(rows);
            for (size_t k = 0; k < rows; k++) {
                const uint32_t l = s.rows.label[k];
                if (l >= nO || pairs[l].x >= nOG)
                    return mfail(m, DEME_ERR_INTERNAL, "%s: a slab's table names the local root %u, which is no vertex", who, l);
                s.rootGid[k] = pairs[l].x;
            }
            return DEME_OK;
        }))
        return rc;
    std::vector<uint32_t> label(nOG, 0xFFFFFFFFu);
    for (uint32_t g = 0; g < nOG; g++)
        if (parent[g] != 0xFFFFFFFFu)
            label[g] = find(g);
    // the merged table, by final label
    std::vector<uint32_t> size(askTable ? nOG : 0, 0u);
    std::vector<double> mass(size.size(), 0.0), moment(3 * size.size(), 0.0);
    for (const SlabRows& s : perSlab)
        for (size_t k = 0; k < s.rootGid.size(); k++) {
            const uint32_t l = label[s.rootGid[k]];
            size[l] += s.rows.size[k], mass[l] += s.rows.mass[k];
            for (int j = 0; j < 3; j++)
                moment[3 * (size_t)l + j] += s.rows.moment[3 * k + j];
        }
    DemeClusterSummary sum{0, edges, 0, 0, 0, 0xFFFFFFFFull};
    size_t rows = 0;
    for (uint32_t g = 0; g < (uint32_t)size.size(); g++) {
        if (!size[g])
            continue;
        rows++;
        sum.vertices += size[g], sum.clusters++, sum.singletons += size[g] == 1;
        if (size[g] > sum.largestSize)  // (labels ascending: the first of the largest size stays)
            sum.largestSize = size[g], sum.largestLabel = g;
    }
    if (nClusters)
        *nClusters = rows;
    if (table && tableCap < rows)
        return mfail(m, DEME_ERR_INVALID, "%s: the table has %zu rows; room for %zu was given", who, rows, tableCap);
    if (summary)
        *summary = sum;
    if (labels && nOG)
        memcpy(labels, label.data(), (size_t)nOG * 4);
    if (table) {
        size_t k = 0;
        for (uint32_t g = 0; g < (uint32_t)size.size(); g++) {
            if (!size[g])
                continue;
            if (table->label)
                table->label[k] = g;
            if (table->size)
                table->size[k] = size[g];
            if (table->mass)
                table->mass[k] = mass[g];
            if (table->moment)
                for (int j = 0; j < 3; j++)
                    table->moment[3 * k + j] = moment[3 * (size_t)g + j];
            k++;
        }
    }
    return DEME_OK;
}

// ---- moving the slab boundaries (load balance of a bed that drifts or piles up) --------------------------------------------------------
// deme_halo_group_migrate keeps the boundaries where the plan put them.  deme_multi_rebalance recomputes them from the clumps'
// CURRENT coordinates -- equal counts again, snapped to bin faces like the plan's -- and lets the same migration move the clumps that
// now lie on the other side of a boundary.  A clump travels to a FACE neighbour only, and the ghost sets are taken from face
// neighbours, so one call moves every boundary by less than the narrower of its two slabs minus the halo (a boundary that wants to go
// further gets there over several calls).
int deme_multi_rebalance(deme_multi* m, uint32_t* clumpsMoved, double* newEdges) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    const uint32_t nSlabs = m->plan->nSlabs;
    if (clumpsMoved)
        *clumpsMoved = 0;
    if (nSlabs < 2)
        return DEME_OK;
    if (int rc = deme_multi_sync(m))
        return rc;
    // the coordinate of every own clump along the cut axis, and the boundaries in force
    const int axis = m->plan->axis;
    std::vector<double> x;
    std::vector<double> edges(nSlabs + 1);
    DemeParams hp{};
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            const SlabGeom& q = r.s->geo;
            if (!q.set)
                return mfail(m, DEME_ERR_INVALID, "rebalance: slab %u has no books", r.no);
            hp = r.c->hp;
            edges[r.no] = q.xLo, edges[r.no + 1] = q.xHi;
            std::vector<OwnerRec> rec(q.nOwn);
            if (q.nOwn && hipMemcpy(rec.data(), r.c->owners.p, (size_t)q.nOwn * sizeof(OwnerRec), hipMemcpyDeviceToHost) != hipSuccess)
                return mfail(m, DEME_ERR_HIP, "rebalance: the owners of slab %u could not be read", r.no);
            for (auto& o : rec)
                x.push_back(decomp_coord(hp, o.voxelID, o.locX, o.locY, o.locZ, axis));
            return DEME_OK;
        }))
        return rc;
    if (x.empty())
        return DEME_OK;
    std::sort(x.begin(), x.end());
    const double lbf = axis == 0 ? (double)hp.LBFX : axis == 1 ? (double)hp.LBFY : (double)hp.LBFZ;
    const double halo = m->plan->halo;
    std::vector<double> want(edges);
    for (uint32_t i = 1; i < nSlabs; i++) {
        const double pos = (double)i / (double)nSlabs * (double)(x.size() - 1);
        const size_t k = (size_t)pos;
        double e = k + 1 < x.size() ? x[k] + (x[k + 1] - x[k]) * (pos - (double)k) : x.back();
        if (hp.binSize > 0)
            e = lbf + std::nearbyint((e - lbf) / hp.binSize) * hp.binSize;
        want[i] = e;
    }
    // one call's reach: a boundary stays inside the band its two slabs leave it (old slab width minus the halo, and a slab never
    // gets thinner than the halo)
    std::vector<double> next(edges);
    for (uint32_t i = 1; i < nSlabs; i++) {
        const double lo = (i == 1 ? edges[i] - 1e300 : edges[i - 1] + halo), hi = (i + 1 == nSlabs ? edges[i] + 1e300 : edges[i + 1] - halo);
        const double wl = (i == 1 ? 1e300 : edges[i] - edges[i - 1]), wr = (i + 1 == nSlabs ? 1e300 : edges[i + 1] - edges[i]);
        const double reach = std::max(0.0, std::min(wl, wr) - halo);
        double e = std::min(std::max(want[i], edges[i] - reach), edges[i] + reach);
        e = std::min(std::max(e, lo), hi);
        next[i] = e;
    }
    for (uint32_t i = 1; i + 1 < nSlabs; i++)  // (an interior slab keeps at least a halo of width: where two boundaries would come
        if (next[i + 1] - next[i] < halo)      // closer than that, both stay where they are this time)
            next[i] = edges[i], next[i + 1] = edges[i + 1];
    for (uint32_t s = 0; s < nSlabs; s++)
        if (HaloSlab* sl = multi_slab(m, s).s)
            sl->geo.xLo = next[s], sl->geo.xHi = next[s + 1];
    for (uint32_t i = 0; i <= nSlabs; i++)
        m->plan->edges[i] = next[i];
    if (newEdges)
        for (uint32_t i = 0; i <= nSlabs; i++)
            newEdges[i] = next[i];
    std::vector<uint32_t> moved(m->groups.size(), 0);
    if (int rc = multi_each(m, [&](deme_halo_group* g, size_t i) { return deme_halo_group_migrate(g, &moved[i]); }))
        return rc;
    uint32_t tot = 0;
    for (uint32_t v : moved)
        tot += v;
    m->clumpsMigrated += tot, m->sinceMigration = 0, m->rowsValid = false;
    m->migrationsSinceRebalance = 0, m->nRebalances++;
    if (clumpsMoved)
        *clumpsMoved = tot;
    return DEME_OK;
}

int deme_multi_slab_counts(deme_multi* m, uint32_t slab, uint32_t counts[6], double range[2]) {
    if (!m || !m->plan || slab >= m->plan->nSlabs)
        return DEME_ERR_INVALID;
    const SlabRef r = multi_slab(m, slab);
    if (!r.s)
        return DEME_ERR_INVALID;
    if (range)
        range[0] = r.s->geo.xLo, range[1] = r.s->geo.xHi;
    return counts ? deme_halo_group_slab_counts(r.g, r.c, counts) : DEME_OK;
}

// deme_change_owner_sizes on a decomposed run, by GLOBAL owner id: every slab resizes its own clumps and its ghost copies of them
// (matched by ownerGid).  Migration carries component indices between slabs, so every slab must hold the same table: the keys of
// all slabs are merged, their uses summed, the table planned once and applied everywhere.  Nothing changes before every check has
// passed -- the ids, the 16-bit index, and the halo the plan was cut with, which must still hold two reaches of the largest clump.
int deme_multi_change_owner_sizes(deme_multi* m, const uint32_t* globalIds, const float* factors, size_t n) {
    if (!m || !m->plan)
        return DEME_ERR_INVALID;
    std::vector<uint32_t> fb;
    char msg[256];
    if (int rc = resize_check(msg, sizeof msg, globalIds, factors, n, m->plan->nOwnersGlobal, fb))
        return mfail(m, rc, "deme_multi_change_owner_sizes: %s", msg);
    if (!n)
        return DEME_OK;
    if (int rc = deme_multi_sync(m))
        return rc;
    std::vector<uint32_t> byGid(m->plan->nOwnersGlobal, 0);
    for (size_t i = 0; i < n; i++)
        byGid[globalIds[i]] = fb[i];
    std::map<uint64_t, uint32_t> merged;  // key -> spheres that carry it, over every slab (own clumps and ghost copies)
    std::vector<uint32_t> usesAll;
    const deme_ctx* first = nullptr;
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int {
            deme_ctx* c = r.c;
            if (!first) {
                first = c;
                usesAll.assign(c->nComp, 0);
            } else if (c->nComp != first->nComp || c->nTemplateComps != first->nTemplateComps ||
                       memcmp(c->hComp.data(), first->hComp.data(), (size_t)c->nComp * sizeof(float4)) != 0) {
                return mfail(m, DEME_ERR_INVALID, "deme_multi_change_owner_sizes: the slabs' component tables differ");
            }
            SlabIds book;
            std::vector<uint32_t> ids, bits;
            if (int rc = slab_ids(m, r, IDS_OWNER, book))
                return rc;
            for (uint32_t i = 0; i < c->nOwnerClumps; i++) {  // own clumps [0, nOwn) and ghost copies [nOwn, nOwnerClumps)
                const uint32_t gid = book.ownerGid[i];
                if (gid < byGid.size() && byGid[gid])
                    ids.push_back(i), bits.push_back(byGid[gid]);
            }
            std::vector<uint64_t> keys;
            std::vector<uint32_t> runs, uses;
            if (int rc = resize_collect(c, ids.data(), bits.data(), ids.size(), keys, runs, uses))
                return rc;
            for (size_t u = 0; u < keys.size(); u++)
                merged[keys[u]] += runs[u];
            for (size_t k = 0; k < uses.size(); k++)
                usesAll[k] += uses[k];
            return DEME_OK;
        }))
        return rc;
    if (merged.empty() || !first)
        return DEME_OK;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> runs;
    for (auto& kv : merged)  // (std::map: sorted, as the apply pass's binary search wants them)
        keys.push_back(kv.first), runs.push_back(kv.second);
    ResizePlan pl;
    resize_plan(first->hComp, first->nTemplateComps, keys, runs, usesAll, pl);
    if (pl.table.size() > 65535)
        return mfail(m, DEME_ERR_INVALID, "deme_multi_change_owner_sizes: the resized scene needs %zu clump components; at most 65535 are "
                     "supported", pl.table.size());
    if (2.0 * pl.reach > m->plan->halo)
        return mfail(m, DEME_ERR_HALO, "deme_multi_change_owner_sizes: the largest clump would reach %g m from its centre, but the slabs were "
                     "cut with a halo of %g m, which must hold two such reaches; build the run again with a halo of at least %g m",
                     pl.reach, m->plan->halo, 2.0 * pl.reach);
    if (int rc = multi_slabs(m, [&](const SlabRef& r) -> int { return resize_apply(r.c, keys, pl); }))
        return rc;
    m->rowsValid = false;
    return DEME_OK;
}

// every sphere's component index by GLOBAL sphere id (a ghost copy holds what its own slab holds)
int deme_multi_download_sphere_components(deme_multi* m, uint16_t* comp, size_t cap) {
    if (!m || !m->plan || !comp)
        return DEME_ERR_INVALID;
    if (cap < m->plan->nSpheresGlobal)
        return mfail(m, DEME_ERR_INVALID, "buffer too small: need %u", m->plan->nSpheresGlobal);
    if (int rc = deme_multi_sync(m))
        return rc;
    return multi_slabs(m, [&](const SlabRef& r) -> int {
        SlabIds ids;
        std::vector<uint16_t> loc(r.c->nSpheres);
        if (int rc = slab_ids(m, r, IDS_SPHERE, ids))
            return rc;
        if (int rc = deme_download_sphere_components(r.c, loc.data(), loc.size()))
            return rc;
        for (uint32_t i = 0; i < r.c->nSpheres; i++)
            if (ids.sphereGid[i] < m->plan->nSpheresGlobal)
                comp[ids.sphereGid[i]] = loc[i];
        return DEME_OK;
    });
}
