// deme_migrate_host.inc -- host orchestration of deme_halo_group_set_slab / deme_halo_group_migrate (included by deme_hip.hip
// inside its extern "C" block; kernels: deme_migrate.h).  Migration is rare (every few thousand steps), so this code prefers
// clarity to overlap: every phase ends on a stream synchronisation, buffers are allocated per call and freed at its end.  What
// must not happen -- and does not -- is a slab's state or history crossing the host: only counts do.

namespace {

struct MigScratch {  // everything one slab allocates during a migration: bump allocation from the slab's pool (MigPool), separate
                     // allocations for what does not fit -- the pool is then regrown before the next migration
    MigPool* pool = nullptr;
    size_t used = 0, need = 0;
    std::vector<void*> owned;
    void bind(MigPool* p) {
        pool = p;
        used = need = 0;
        if (p->lastNeed > p->cap) {
            if (p->base)
                hipFree(p->base);
            p->base = nullptr;
            p->cap = p->lastNeed + p->lastNeed / 4;
            if (hipMalloc(&p->base, p->cap) != hipSuccess)
                p->base = nullptr, p->cap = 0;
        }
    }
    void* alloc(size_t bytes) {
        const size_t b = (std::max<size_t>(bytes, 256) + 255) & ~(size_t)255;
        need += b;
        if (pool && pool->base && used + b <= pool->cap) {
            void* p = (char*)pool->base + used;
            used += b;
            return p;
        }
        void* p = nullptr;
        if (hipMalloc(&p, b) != hipSuccess)
            return nullptr;
        owned.push_back(p);
        return p;
    }
    ~MigScratch() {
        for (void* p : owned)
            hipFree(p);
        if (pool)
            pool->lastNeed = std::max(pool->lastNeed, need);
    }
};

#define MIGCK(call)                                                                                                     \
    do {                                                                                                                \
        hipError_t _e = (call);                                                                                         \
        if (_e != hipSuccess)                                                                                           \
            return gfail(g, DEME_ERR_HIP, "migrate: %s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

int mig_scan_u32(deme_halo_group* g, deme_ctx* c, const uint32_t* in, uint32_t* out, size_t n) {  // exclusive plus-scan on the slab's stream
    if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, in, out, 0u, n, rocprim::plus<uint32_t>(), c->stream);
        }))
        return gfail(g, rc, "migrate: %s", c->err.c_str());
    return DEME_OK;
}
int mig_scan_count(deme_halo_group* g, deme_ctx* c, const MigCount* in, MigCount* out, size_t n) {
    if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, in, out, MigCount{}, n, MigCountPlus(), c->stream);
        }))
        return gfail(g, rc, "migrate: %s", c->err.c_str());
    return DEME_OK;
}

// what the per-owner / per-sphere scratch of a context has to hold for new counts (the allocation half of deme_upload_scene)
int mig_scratch_for_counts(deme_ctx* c, size_t nO, size_t nS) {
    if (int rc = owner_scratch_for_counts(c, nO))
        return rc;
    if (int rc = sphere_scratch_for_counts(c, nS))
        return rc;
    if (c->incCap < 8 * nS)
        if (int rc = grow_incidence_arena(c, std::max<size_t>(8 * nS, 4096)))
            return rc;
    if (c->cntCap < 6 * nS)
        if (int rc = grow_contact_arena(c, std::max<size_t>(6 * nS, 4096)))
            return rc;
    if (c->asyncLead && c->ownersSnap.p)
        if (int rc = ensure(c, c->ownersSnap, nO * sizeof(OwnerRec)))
            return rc;
    return DEME_OK;
}

struct MigSlabWork {  // host-side state of one slab across the phases
    MigScratch mem;
    uint32_t nO = 0, nClumps = 0, nS = 0, nX = 0, nW = 0;
    uint32_t nOW = 0, nGW = 0;  // user owner / sphere wildcard arrays carried along
    MigWcPtrs oldOW{}, oldGW{}, ownOW{}, ownGW{};  // the context's arrays; the own section of the re-assembled slab
    uint64_t nC = 0;
    uint32_t *firstSph = nullptr, *toL = nullptr, *toR = nullptr, *posL = nullptr, *posR = nullptr;
    uint8_t* dest = nullptr;
    MigCount *cnt = nullptr, *pos = nullptr;
    MigCount tot{};
    MigRowHead* rowH = nullptr;
    float* rowW = nullptr;
    MigBuf send[2], recv[2], gsend[2], grecv[2];
    // own stage of the re-assembled slab
    OwnerRec* ownOwners = nullptr;
    SphereRec* ownSpheres = nullptr;
    uint32_t *ownGid = nullptr, *ownSGid = nullptr, *ownFirst = nullptr;
    uint32_t nOwnNew = 0, sOwnNew = 0;
    uint32_t* sendIds[2] = {nullptr, nullptr};
};

int mig_alloc_buf(deme_halo_group* g, MigScratch& mem, MigBuf& b, uint32_t nW, uint32_t nOW, uint32_t nGW) {
    b.owc = mem.alloc((size_t)b.nC * std::max(nOW, 1u) * 4);
    b.swc = mem.alloc((size_t)b.nS * std::max(nGW, 1u) * 4);
    if (!b.owc || !b.swc)
        return gfail(g, DEME_ERR_HIP, "migrate: out of device memory for an exchange buffer");
    b.clumps = mem.alloc((size_t)b.nC * sizeof(MigClump));
    b.spheres = mem.alloc((size_t)b.nS * sizeof(MigSphere));
    b.rowH = mem.alloc((size_t)b.nR * sizeof(MigRowHead));
    b.rowW = mem.alloc((size_t)b.nR * std::max(nW, 1u) * 4);
    if (!b.clumps || !b.spheres || !b.rowH || !b.rowW)
        return gfail(g, DEME_ERR_HIP, "migrate: out of device memory for an exchange buffer");
    return DEME_OK;
}

// one exchange round: every slab's send[k] goes to its neighbour's recv[1 - k].  Local neighbours borrow the sender's buffers;
// remote ones get the counts first, then the payload, over the group's communicator.
// A migration is a collective: a rank that found a local reason to give up (a clump outside the decomposed range, a scene the
// migration does not carry, no memory) must not leave its neighbours waiting in the receives of mig_exchange.  Before every
// exchange the ranks add up their error flags; if any is set they all return.  (One rank: nothing to agree on.)
int mig_agree(deme_halo_group* g, int localRc, const char* where) {
    if (g->world <= 1)
        return localRc;
    if (!g->agreeBuf && hipMalloc(&g->agreeBuf, 16) != hipSuccess)
        g->agreeBuf = nullptr;  // (cannot even allocate 16 bytes: fall through to the local code; the others time out in RCCL)
    float flag = localRc ? 1.f : 0.f, total = flag;
    if (g->agreeBuf) {
        GHIP(hipMemcpy(g->agreeBuf, &flag, 4, hipMemcpyHostToDevice));
        GNCCL(g->api->AllReduce(g->agreeBuf, g->agreeBuf, 1, kNcclFloat32, kNcclSum, g->comm, g->xstream));
        GHIP(hipStreamSynchronize(g->xstream));
        GHIP(hipMemcpy(&total, g->agreeBuf, 4, hipMemcpyDeviceToHost));
    }
    if (localRc)
        return localRc;
    if (total > 0.f)
        return gfail(g, DEME_ERR_PEER, "migrate: %d other rank(s) gave up %s; this rank returns with them (state untouched)", (int)total, where);
    return DEME_OK;
}

// does ANY rank say yes?  (one all-reduce of a flag; one rank: its own answer)
int mig_any(deme_halo_group* g, bool local, bool& any) {
    any = local;
    if (g->world <= 1)
        return DEME_OK;
    if (!g->agreeBuf)
        GHIP(hipMalloc(&g->agreeBuf, 16));
    float flag = local ? 1.f : 0.f;
    GHIP(hipMemcpy(g->agreeBuf, &flag, 4, hipMemcpyHostToDevice));
    GNCCL(g->api->AllReduce(g->agreeBuf, g->agreeBuf, 1, kNcclFloat32, kNcclSum, g->comm, g->xstream));
    GHIP(hipStreamSynchronize(g->xstream));
    GHIP(hipMemcpy(&flag, g->agreeBuf, 4, hipMemcpyDeviceToHost));
    any = flag > 0.f;
    return DEME_OK;
}

int mig_exchange(deme_halo_group* g, std::vector<MigSlabWork>& W, bool ghosts) {
    auto find = [&](deme_ctx* c) -> int {
        for (size_t i = 0; i < g->slabs.size(); i++)
            if (g->slabs[i].ctx == c)
                return (int)i;
        return -1;
    };
    for (auto& s : g->slabs)
        GHIP(hipStreamSynchronize(s.ctx->stream));
    bool anyRemote = false;
    for (size_t i = 0; i < g->slabs.size(); i++)
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = g->slabs[i].side[k];
            MigBuf& rb = ghosts ? W[i].grecv[k] : W[i].recv[k];
            rb = MigBuf{};
            if (sd.peerRank < 0)
                continue;
            if (sd.peerLocal) {
                const int j = find(sd.peerLocal);
                if (j < 0)
                    return gfail(g, DEME_ERR_INVALID, "migrate: a local neighbour context is not attached to the group");
                rb = ghosts ? W[j].gsend[1 - k] : W[j].send[1 - k];
                rb.borrowed = true;
            } else {
                anyRemote = true;
            }
        }
    if (!anyRemote)
        return DEME_OK;
#define GNCCL_IN_GROUP(call)                                                                                                     \
    do {                                                                                                                         \
        int _r = (call);                                                                                                         \
        if (_r != 0) {                                                                                                           \
            g->api->GroupEnd();                                                                                                  \
            return gfail(g, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, g->api->GetErrorString(_r), __FILE__, __LINE__);        \
        }                                                                                                                        \
    } while (0)
    // counts (their 16-byte device words are set aside first: nothing inside the RCCL group can fail for a local reason)
    int rcLocal = DEME_OK;
    for (size_t i = 0; i < g->slabs.size() && !rcLocal; i++)
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = g->slabs[i].side[k];
            if (sd.peerRank < 0 || sd.peerLocal)
                continue;
            MigBuf& sb = ghosts ? W[i].gsend[k] : W[i].send[k];
            MigBuf& rb = ghosts ? W[i].grecv[k] : W[i].recv[k];
            const uint32_t h[3] = {sb.nC, sb.nS, sb.nR};
            sb.counts = W[i].mem.alloc(16), rb.counts = W[i].mem.alloc(16);
            if (!sb.counts || !rb.counts || hipMemcpy(sb.counts, h, 12, hipMemcpyHostToDevice) != hipSuccess) {
                rcLocal = gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
                break;
            }
        }
    if (int rc = mig_agree(g, rcLocal, "before the count handshake"))
        return rc;
    GNCCL(g->api->GroupStart());
    for (size_t i = 0; i < g->slabs.size(); i++)
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = g->slabs[i].side[k];
            if (sd.peerRank < 0 || sd.peerLocal)
                continue;
            MigBuf& sb = ghosts ? W[i].gsend[k] : W[i].send[k];
            MigBuf& rb = ghosts ? W[i].grecv[k] : W[i].recv[k];
            GNCCL_IN_GROUP(g->api->Send(sb.counts, 12, kNcclUint8, sd.peerRank, g->comm, g->xstream));
            GNCCL_IN_GROUP(g->api->Recv(rb.counts, 12, kNcclUint8, sd.peerRank, g->comm, g->xstream));
        }
    GNCCL(g->api->GroupEnd());
    GHIP(hipStreamSynchronize(g->xstream));
    for (size_t i = 0; i < g->slabs.size() && !rcLocal; i++)
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = g->slabs[i].side[k];
            if (sd.peerRank < 0 || sd.peerLocal)
                continue;
            MigBuf& rb = ghosts ? W[i].grecv[k] : W[i].recv[k];
            uint32_t h[3];
            if (hipMemcpy(h, rb.counts, 12, hipMemcpyDeviceToHost) != hipSuccess) {
                rcLocal = gfail(g, DEME_ERR_HIP, "migrate: reading the neighbour's counts failed");
                break;
            }
            rb.nC = h[0], rb.nS = h[1], rb.nR = h[2];
            if ((rcLocal = mig_alloc_buf(g, W[i].mem, rb, W[i].nW, W[i].nOW, W[i].nGW)) != 0)
                break;
        }
    if (int rc = mig_agree(g, rcLocal, "sizing its receive buffers"))  // (a rank without room for what it is about to receive)
        return rc;
    // payloads
    GNCCL(g->api->GroupStart());
    for (size_t i = 0; i < g->slabs.size(); i++)
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = g->slabs[i].side[k];
            if (sd.peerRank < 0 || sd.peerLocal)
                continue;
            MigBuf& sb = ghosts ? W[i].gsend[k] : W[i].send[k];
            MigBuf& rb = ghosts ? W[i].grecv[k] : W[i].recv[k];
            const uint32_t nW = std::max(W[i].nW, 1u);
            if (sb.nC) {
                GNCCL_IN_GROUP(g->api->Send(sb.clumps, (size_t)sb.nC * sizeof(MigClump), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                GNCCL_IN_GROUP(g->api->Send(sb.spheres, (size_t)sb.nS * sizeof(MigSphere), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                if (W[i].nOW)
                    GNCCL_IN_GROUP(g->api->Send(sb.owc, (size_t)sb.nC * W[i].nOW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
                if (W[i].nGW && sb.nS)
                    GNCCL_IN_GROUP(g->api->Send(sb.swc, (size_t)sb.nS * W[i].nGW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
            }
            if (sb.nR) {
                GNCCL_IN_GROUP(g->api->Send(sb.rowH, (size_t)sb.nR * sizeof(MigRowHead), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                GNCCL_IN_GROUP(g->api->Send(sb.rowW, (size_t)sb.nR * nW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
            }
            if (rb.nC) {
                GNCCL_IN_GROUP(g->api->Recv(rb.clumps, (size_t)rb.nC * sizeof(MigClump), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                GNCCL_IN_GROUP(g->api->Recv(rb.spheres, (size_t)rb.nS * sizeof(MigSphere), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                if (W[i].nOW)
                    GNCCL_IN_GROUP(g->api->Recv(rb.owc, (size_t)rb.nC * W[i].nOW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
                if (W[i].nGW && rb.nS)
                    GNCCL_IN_GROUP(g->api->Recv(rb.swc, (size_t)rb.nS * W[i].nGW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
            }
            if (rb.nR) {
                GNCCL_IN_GROUP(g->api->Recv(rb.rowH, (size_t)rb.nR * sizeof(MigRowHead), kNcclUint8, sd.peerRank, g->comm, g->xstream));
                GNCCL_IN_GROUP(g->api->Recv(rb.rowW, (size_t)rb.nR * nW * 4, kNcclUint8, sd.peerRank, g->comm, g->xstream));
            }
        }
    GNCCL(g->api->GroupEnd());
#undef GNCCL_IN_GROUP
    GHIP(hipStreamSynchronize(g->xstream));
    return DEME_OK;
}

}  // namespace

int deme_halo_group_set_slab(deme_halo_group* g, deme_ctx* c, const uint32_t* ownerGlobal, const uint32_t* sphereGlobal, uint32_t nOwn,
                             uint32_t nGhostLeft, uint32_t nGhostRight, double xLo, double xHi, double halo, uint32_t flipMask) {
    if (!g || !c || !ownerGlobal || !sphereGlobal)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    for (auto& s : g->slabs)
        if (s.ctx == c) {
            // (a slab WITH neighbours keeps the decomposition's order: its exchange lists and books name slots.  A chain of one
            // slab has nothing to exchange or migrate -- its context is a plain one and may keep the engine's order: the books
            // then serve deme_halo_group_download_state / _upload_state only, in the caller's ids like every id at the boundary)
            if (c->permuted && (s.side[0].peerRank >= 0 || s.side[1].peerRank >= 0))
                return gfail(g, DEME_ERR_INVALID, "set_slab: the context keeps an order of its own (a scene without ghosts uploaded in the fast mode); a slab's order is the decomposition's");
            if (nOwn + nGhostLeft + nGhostRight != c->nOwnerClumps)
                return gfail(g, DEME_ERR_INVALID, "set_slab: %u own + %u + %u ghost clumps, the scene has %u clumps", nOwn, nGhostLeft,
                             nGhostRight, c->nOwnerClumps);
            SlabGeom& q = s.geo;
            if (q.ownerGid)
                hipFree(q.ownerGid);
            if (q.sphereGid)
                hipFree(q.sphereGid);
            GHIP(hipMalloc(&q.ownerGid, std::max<size_t>(c->nOwners, 1) * 4));
            GHIP(hipMalloc(&q.sphereGid, std::max<size_t>(c->nSpheres, 1) * 4));
            GHIP(hipMemcpy(q.ownerGid, ownerGlobal, (size_t)c->nOwners * 4, hipMemcpyHostToDevice));
            GHIP(hipMemcpy(q.sphereGid, sphereGlobal, (size_t)c->nSpheres * 4, hipMemcpyHostToDevice));
            q.xLo = xLo, q.xHi = xHi, q.halo = halo, q.nOwn = nOwn, q.nGL = nGhostLeft, q.nGR = nGhostRight, q.flipMask = flipMask;
            q.set = true;
            return DEME_OK;
        }
    return gfail(g, DEME_ERR_INVALID, "set_slab: the context is not attached to the group");
}

int deme_halo_group_slab_counts(const deme_halo_group* g, const deme_ctx* c, uint32_t counts[6]) {
    if (!g || !c || !counts)
        return DEME_ERR_INVALID;
    for (auto& s : g->slabs)
        if (s.ctx == c) {
            counts[0] = s.geo.nOwn, counts[1] = s.geo.nGL, counts[2] = s.geo.nGR;
            counts[3] = c->nOwners, counts[4] = c->nSpheres, counts[5] = (uint32_t)c->nContacts;
            return DEME_OK;
        }
    return DEME_ERR_INVALID;
}

namespace {
// A slab's id books on the host -- the global id of every owner slot and of every sphere, every sphere's owner slot and component --,
// only the arrays that are asked for (null: not read).  The ONE host reader of the books: the caller has selected the slab's device
// and waited for whatever writes them (a migration).
hipError_t slab_ids_host(const HaloSlab& s, uint32_t* ownerGlobal, uint32_t* sphereGlobal, uint32_t* sphereOwner, uint16_t* sphereComp) {
    const deme_ctx* c = s.ctx;
    hipError_t e = hipSuccess;
    if (ownerGlobal && c->nOwners)
        e = hipMemcpy(ownerGlobal, s.geo.ownerGid, (size_t)c->nOwners * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sphereGlobal && c->nSpheres)
        e = hipMemcpy(sphereGlobal, s.geo.sphereGid, (size_t)c->nSpheres * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && (sphereOwner || sphereComp) && c->nSpheres) {
        std::vector<SphereRec> h(c->nSpheres);
        e = hipMemcpy(h.data(), c->spheres.p, (size_t)c->nSpheres * sizeof(SphereRec), hipMemcpyDeviceToHost);
        for (uint32_t i = 0; e == hipSuccess && i < c->nSpheres; i++) {
            if (sphereOwner)
                sphereOwner[i] = h[i].owner;
            if (sphereComp)
                sphereComp[i] = h[i].comp;
        }
    }
    return e;
}
}  // namespace

int deme_halo_group_download_ids(deme_halo_group* g, deme_ctx* c, uint32_t* ownerGlobal, uint32_t* sphereGlobal, uint32_t* sphereOwner,
                                 uint16_t* sphereComp) {
    if (!g || !c)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    for (auto& s : g->slabs)
        if (s.ctx == c && s.geo.set) {
            GHIP(hipStreamSynchronize(c->stream));
            GHIP(slab_ids_host(s, ownerGlobal, sphereGlobal, sphereOwner, sphereComp));
            return DEME_OK;
        }
    return gfail(g, DEME_ERR_INVALID, "download_ids: the context has no slab geometry (deme_halo_group_set_slab)");
}

int deme_halo_group_migrate(deme_halo_group* g, uint32_t* clumpsMoved) {
    if (!g || !g->comm)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    const size_t nSl = g->slabs.size();
    std::vector<MigSlabWork> W(nSl);
    uint32_t moved = 0;
    {   // persistent marks travel in the history rows: every slab of every rank has to know whether any are about
        bool localAny = false;
        for (auto& sl : g->slabs)
            localAny = localAny || !sl.ctx->hPersist.empty();
        if (int rc = mig_any(g, localAny, g->anyPersist))
            return rc;
    }
    // ---- phase A: who leaves, with which rows.  (A lambda: a local failure is agreed upon with the other ranks below instead of
    // leaving them in the exchange's receives.)
    auto phaseA = [&]() -> int {
    for (size_t i = 0; i < nSl; i++) {
        HaloSlab& sl = g->slabs[i];
        deme_ctx* c = sl.ctx;
        SlabGeom& q = sl.geo;
        MigSlabWork& w = W[i];
        w.mem.bind(&sl.pool);
        if (!q.set)
            return gfail(g, DEME_ERR_INVALID, "migrate: a slab has no geometry (deme_halo_group_set_slab)");
        if (c->permuted)
            return gfail(g, DEME_ERR_INVALID, "migrate: a slab without neighbours keeps the engine's order; there is nowhere to migrate to");
        // user wildcard arrays (owner and sphere kinds: triangles and analytical components do not migrate) travel with the clumps;
        // every slab of every rank has to hold the same model, or the packets would not match
        w.nOW = c->nOwnerWc, w.nGW = c->nGeoWc;
        if (w.nOW > 8 || w.nGW > 8)
            return gfail(g, DEME_ERR_INVALID, "migrate: more than 8 wildcard arrays of a kind");
        if (i && (w.nOW != W[0].nOW || w.nGW != W[0].nGW))
            return gfail(g, DEME_ERR_INVALID, "migrate: the slabs hold force models with different owner / geometry wildcards (%u / %u and %u / %u)",
                         W[0].nOW, W[0].nGW, w.nOW, w.nGW);
        for (uint32_t k = 0; k < w.nOW; k++)
            if (!(w.oldOW.p[k] = c->userWc[0][k].as<float>()) && c->nOwners)
                return gfail(g, DEME_ERR_INVALID, "migrate: owner wildcard array %u does not exist", k);
        for (uint32_t k = 0; k < w.nGW; k++)
            if (!(w.oldGW.p[k] = c->userWc[1][k].as<float>()) && c->nSpheres)
                return gfail(g, DEME_ERR_INVALID, "migrate: sphere wildcard array %u does not exist", k);
        if (c->mapFresh)
            if (int rc = do_migrate(c))
                return gfail(g, rc, "migrate: %s", c->err.c_str());
        GHIP(hipStreamSynchronize(c->stream));
        if (c->haloStream)
            GHIP(hipStreamSynchronize(c->haloStream));
        w.nO = c->nOwners, w.nClumps = c->nOwnerClumps, w.nS = c->nSpheres, w.nX = c->nOwners - c->nOwnerClumps;
        w.nW = c->hp.nContactWildcards;
        w.nC = c->haveList ? c->nContacts : 0;
        if (w.nW > DEME_MIG_MAXW)
            return gfail(g, DEME_ERR_INVALID, "migrate: more than %u contact wildcards", DEME_MIG_MAXW);
        w.firstSph = (uint32_t*)w.mem.alloc(((size_t)w.nO + 2) * 4);
        w.dest = (uint8_t*)w.mem.alloc((size_t)w.nClumps + 1);
        w.cnt = (MigCount*)w.mem.alloc(((size_t)w.nClumps + 1) * sizeof(MigCount));
        w.pos = (MigCount*)w.mem.alloc(((size_t)w.nClumps + 1) * sizeof(MigCount));
        if (!w.firstSph || !w.dest || !w.cnt || !w.pos)
            return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        const double inf = std::numeric_limits<double>::infinity();
        const double xLo = sl.side[0].peerRank >= 0 ? q.xLo : -inf, xHi = sl.side[1].peerRank >= 0 ? q.xHi : inf;
        hipLaunchKernelGGL(k_mig_first_sphere, dim3(grid_for(std::max<size_t>(w.nS, (size_t)w.nO + 1))), dim3(256), 0, c->stream, w.nS,
                           c->spheres.as<SphereRec>(), w.nO, w.firstSph);
        hipLaunchKernelGGL(k_mig_classify, dim3(grid_for((size_t)w.nClumps + 1)), dim3(256), 0, c->stream, c->dp, c->owners.as<OwnerRec>(),
                           q.nOwn, w.nClumps, g->axis, xLo, xHi, w.firstSph, w.dest, w.cnt);
        if (int rc = mig_scan_count(g, c, w.cnt, w.pos, (size_t)w.nClumps + 1))
            return rc;
        GHIP(hipMemcpyAsync(&w.tot, w.pos + w.nClumps, sizeof(MigCount), hipMemcpyDeviceToHost, c->stream));
        // rows
        const uint32_t nC = (uint32_t)w.nC, nWs = std::max(w.nW, 1u);
        w.rowH = (MigRowHead*)w.mem.alloc((size_t)nC * sizeof(MigRowHead));
        w.rowW = (float*)w.mem.alloc((size_t)nC * nWs * 4);
        w.toL = (uint32_t*)w.mem.alloc(((size_t)nC + 1) * 4), w.toR = (uint32_t*)w.mem.alloc(((size_t)nC + 1) * 4);
        w.posL = (uint32_t*)w.mem.alloc(((size_t)nC + 1) * 4), w.posR = (uint32_t*)w.mem.alloc(((size_t)nC + 1) * 4);
        if (!w.rowH || !w.rowW || !w.toL || !w.toR || !w.posL || !w.posR)
            return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        hipLaunchKernelGGL(k_mig_rows, dim3(grid_for((size_t)nC + 1)), dim3(256), 0, c->stream, nC, w.nW, q.flipMask,
                           c->keysSorted[c->keysCur].as<uint64_t>(), c->wc[c->wcCur].as<float>(), c->spheres.as<SphereRec>(),
                           (const uint32_t*)q.sphereGid, w.dest, w.nClumps, w.rowH, w.rowW, w.toL, w.toR,
                           c->hPersist.empty() ? (const uint64_t*)nullptr : c->persistKeys.as<uint64_t>(), (uint32_t)c->hPersist.size());
        if (int rc = mig_scan_u32(g, c, w.toL, w.posL, (size_t)nC + 1))
            return rc;
        if (int rc = mig_scan_u32(g, c, w.toR, w.posR, (size_t)nC + 1))
            return rc;
        uint32_t nRow[2] = {0, 0};
        GHIP(hipMemcpyAsync(&nRow[0], w.posL + nC, 4, hipMemcpyDeviceToHost, c->stream));
        GHIP(hipMemcpyAsync(&nRow[1], w.posR + nC, 4, hipMemcpyDeviceToHost, c->stream));
        GHIP(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; k++) {
            MigBuf& b = w.send[k];
            b.nC = w.tot.c[k + 1], b.nS = w.tot.s[k + 1], b.nR = nRow[k];
            if (sl.side[k].peerRank < 0 && b.nC)
                return gfail(g, DEME_ERR_INVALID, "migrate: %u clump(s) left the decomposed range", b.nC);
            moved += b.nC;
            if (int rc = mig_alloc_buf(g, w.mem, b, w.nW, w.nOW, w.nGW))
                return rc;
            if (b.nC)
                hipLaunchKernelGGL(k_mig_pack_clumps, dim3(grid_for(w.nClumps)), dim3(256), 0, c->stream, w.nClumps, c->owners.as<OwnerRec>(),
                                   c->spheres.as<SphereRec>(), (const uint32_t*)q.ownerGid, (const uint32_t*)q.sphereGid, w.firstSph, w.dest,
                                   w.pos, (uint32_t)(k + 1), (MigClump*)b.clumps, (MigSphere*)b.spheres);
            if (b.nC && (w.nOW || w.nGW))
                hipLaunchKernelGGL(k_mig_pack_wc, dim3(grid_for(w.nClumps)), dim3(256), 0, c->stream, w.nClumps, w.dest, w.pos, (uint32_t)(k + 1), 0,
                                   w.firstSph, w.nOW, w.nGW, w.oldOW, w.oldGW, (float*)b.owc, (float*)b.swc);
            if (b.nR)
                hipLaunchKernelGGL(k_mig_pack_rows, dim3(grid_for(nC)), dim3(256), 0, c->stream, nC, w.nW, w.rowH, w.rowW, k ? w.toR : w.toL,
                                   k ? w.posR : w.posL, (MigRowHead*)b.rowH, (float*)b.rowW);
        }
    }
    return DEME_OK;
    };
    if (int rc = mig_agree(g, phaseA(), "while selecting its leavers"))
        return rc;
    // ---- phase B: the migrants travel
    if (int rc = mig_exchange(g, W, false))
        return rc;
    // ---- phase C: the own section of every re-assembled slab, and its ghost packets
    auto phaseC = [&]() -> int {
    for (size_t i = 0; i < nSl; i++) {
        HaloSlab& sl = g->slabs[i];
        deme_ctx* c = sl.ctx;
        SlabGeom& q = sl.geo;
        MigSlabWork& w = W[i];
        const uint32_t nStay = w.tot.c[0], sStay = w.tot.s[0];
        w.nOwnNew = nStay + w.recv[0].nC + w.recv[1].nC;
        w.sOwnNew = sStay + w.recv[0].nS + w.recv[1].nS;
        w.ownOwners = (OwnerRec*)w.mem.alloc((size_t)w.nOwnNew * sizeof(OwnerRec));
        w.ownSpheres = (SphereRec*)w.mem.alloc((size_t)w.sOwnNew * sizeof(SphereRec));
        w.ownGid = (uint32_t*)w.mem.alloc((size_t)w.nOwnNew * 4), w.ownSGid = (uint32_t*)w.mem.alloc((size_t)w.sOwnNew * 4);
        w.ownFirst = (uint32_t*)w.mem.alloc(((size_t)w.nOwnNew + 2) * 4);
        MigClump* stayC = (MigClump*)w.mem.alloc((size_t)nStay * sizeof(MigClump));
        MigSphere* stayS = (MigSphere*)w.mem.alloc((size_t)sStay * sizeof(MigSphere));
        float* stayOW = (float*)w.mem.alloc((size_t)nStay * std::max(w.nOW, 1u) * 4);
        float* staySW = (float*)w.mem.alloc((size_t)sStay * std::max(w.nGW, 1u) * 4);
        if (!stayOW || !staySW)
            return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        for (uint32_t k = 0; k < w.nOW; k++)
            if (!(w.ownOW.p[k] = (float*)w.mem.alloc((size_t)w.nOwnNew * 4)))
                return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        for (uint32_t k = 0; k < w.nGW; k++)
            if (!(w.ownGW.p[k] = (float*)w.mem.alloc((size_t)w.sOwnNew * 4)))
                return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        if (!w.ownOwners || !w.ownSpheres || !w.ownGid || !w.ownSGid || !w.ownFirst || !stayC || !stayS)
            return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        // the staying clumps go through the same packet form (one code path for all sections)
        if (nStay)
            hipLaunchKernelGGL(k_mig_pack_clumps, dim3(grid_for(w.nClumps)), dim3(256), 0, c->stream, w.nClumps, c->owners.as<OwnerRec>(),
                               c->spheres.as<SphereRec>(), (const uint32_t*)q.ownerGid, (const uint32_t*)q.sphereGid, w.firstSph, w.dest, w.pos,
                               0u, stayC, stayS);
        if (nStay && (w.nOW || w.nGW))
            hipLaunchKernelGGL(k_mig_pack_wc, dim3(grid_for(w.nClumps)), dim3(256), 0, c->stream, w.nClumps, w.dest, w.pos, 0u, 0, w.firstSph, w.nOW,
                               w.nGW, w.oldOW, w.oldGW, stayOW, staySW);
        struct Sec {
            const MigClump* cl;
            const MigSphere* sp;
            uint32_t n, ns;
            const float *ow, *sw;
        } secs[3] = {{stayC, stayS, nStay, sStay, stayOW, staySW},
                     {(const MigClump*)w.recv[0].clumps, (const MigSphere*)w.recv[0].spheres, w.recv[0].nC, w.recv[0].nS, (const float*)w.recv[0].owc,
                      (const float*)w.recv[0].swc},
                     {(const MigClump*)w.recv[1].clumps, (const MigSphere*)w.recv[1].spheres, w.recv[1].nC, w.recv[1].nS, (const float*)w.recv[1].owc,
                      (const float*)w.recv[1].swc}};
        uint32_t ob = 0, sb = 0;
        for (auto& sc : secs) {
            if (sc.n) {
                uint32_t* ns = (uint32_t*)w.mem.alloc(((size_t)sc.n + 1) * 4);
                uint32_t* off = (uint32_t*)w.mem.alloc(((size_t)sc.n + 1) * 4);
                if (!ns || !off)
                    return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
                hipLaunchKernelGGL(k_mig_nsph, dim3(grid_for((size_t)sc.n + 1)), dim3(256), 0, c->stream, sc.n, sc.cl, ns);
                if (int rc = mig_scan_u32(g, c, ns, off, (size_t)sc.n + 1))
                    return rc;
                hipLaunchKernelGGL(k_mig_unpack, dim3(grid_for(sc.n)), dim3(256), 0, c->stream, sc.n, sc.cl, sc.sp, off, ob, sb, 0u, w.ownOwners,
                                   w.ownSpheres, w.ownGid, w.ownSGid);
                if (w.nOW || w.nGW)
                    hipLaunchKernelGGL(k_mig_unpack_wc, dim3(grid_for(sc.n)), dim3(256), 0, c->stream, sc.n, sc.ow, sc.sw, off, ob, sb, w.nOW, w.nGW,
                                       w.ownOW, w.ownGW);
            }
            ob += sc.n, sb += sc.ns;
        }
        hipLaunchKernelGGL(k_mig_first_sphere, dim3(grid_for(std::max<size_t>(w.sOwnNew, (size_t)w.nOwnNew + 1))), dim3(256), 0, c->stream,
                           w.sOwnNew, w.ownSpheres, w.nOwnNew, w.ownFirst);
        // ghost packets for the neighbours
        uint8_t* gd = (uint8_t*)w.mem.alloc((size_t)w.nOwnNew + 1);
        MigCount* gc = (MigCount*)w.mem.alloc(((size_t)w.nOwnNew + 1) * sizeof(MigCount));
        MigCount* gp = (MigCount*)w.mem.alloc(((size_t)w.nOwnNew + 1) * sizeof(MigCount));
        if (!gd || !gc || !gp)
            return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
        hipLaunchKernelGGL(k_mig_ghost_flags, dim3(grid_for((size_t)w.nOwnNew + 1)), dim3(256), 0, c->stream, c->dp, w.ownOwners, w.nOwnNew, g->axis, q.xLo,
                           q.xHi, q.halo, sl.side[0].peerRank >= 0 ? 1 : 0, sl.side[1].peerRank >= 0 ? 1 : 0, w.ownFirst, gd, gc);
        if (int rc = mig_scan_count(g, c, gc, gp, (size_t)w.nOwnNew + 1))
            return rc;
        MigCount gt{};
        GHIP(hipMemcpyAsync(&gt, gp + w.nOwnNew, sizeof(MigCount), hipMemcpyDeviceToHost, c->stream));
        GHIP(hipStreamSynchronize(c->stream));
        for (int k = 0; k < 2; k++) {
            MigBuf& b = w.gsend[k];
            b.nC = gt.c[k + 1], b.nS = gt.s[k + 1], b.nR = 0;
            if (int rc = mig_alloc_buf(g, w.mem, b, w.nW, w.nOW, w.nGW))
                return rc;
            w.sendIds[k] = (uint32_t*)w.mem.alloc((size_t)std::max(b.nC, 1u) * 4);
            if (!w.sendIds[k])
                return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
            if (b.nC)
                hipLaunchKernelGGL(k_mig_pack_ghosts, dim3(grid_for(w.nOwnNew)), dim3(256), 0, c->stream, w.nOwnNew, w.ownOwners, w.ownSpheres,
                                   w.ownGid, w.ownSGid, w.ownFirst, gd, gp, (uint32_t)(k + 1), (MigClump*)b.clumps, (MigSphere*)b.spheres,
                                   w.sendIds[k]);
            if (b.nC && (w.nOW || w.nGW))
                hipLaunchKernelGGL(k_mig_pack_wc, dim3(grid_for(w.nOwnNew)), dim3(256), 0, c->stream, w.nOwnNew, gd, gp, (uint32_t)(k + 1), 1, w.ownFirst,
                                   w.nOW, w.nGW, w.ownOW, w.ownGW, (float*)b.owc, (float*)b.swc);
        }
    }
    return DEME_OK;
    };
    if (int rc = mig_agree(g, phaseC(), "while assembling its own clumps"))
        return rc;
    // ---- phase D: the ghosts travel
    if (int rc = mig_exchange(g, W, true))
        return rc;
    // ---- phase E: the slabs re-assembled, their history re-seeded, their exchange lists renewed
    for (size_t i = 0; i < nSl; i++) {
        HaloSlab& sl = g->slabs[i];
        deme_ctx* c = sl.ctx;
        SlabGeom& q = sl.geo;
        MigSlabWork& w = W[i];
        const uint32_t nGL = w.grecv[0].nC, nGR = w.grecv[1].nC, sGL = w.grecv[0].nS, sGR = w.grecv[1].nS;
        const uint32_t nClNew = w.nOwnNew + nGL + nGR, nONew = nClNew + w.nX, nSNew = w.sOwnNew + sGL + sGR;
        if ((uint64_t)nSNew >= (1ull << 31) || nONew >= (1u << 30))
            return gfail(g, DEME_ERR_INVALID, "migrate: the re-assembled slab is too large for the id fields");
        // new arrays (the old ones are still read: extras, and the rows were taken from the old list already)
        DevBuf newOwners, newSpheres;
        void *newOGid = nullptr, *newSGid = nullptr;
        MIGCK(hipMalloc(&newOwners.p, std::max<size_t>(nONew, 1) * sizeof(OwnerRec)));
        newOwners.bytes = std::max<size_t>(nONew, 1) * sizeof(OwnerRec);
        MIGCK(hipMalloc(&newSpheres.p, std::max<size_t>(nSNew, 1) * sizeof(SphereRec)));
        newSpheres.bytes = std::max<size_t>(nSNew, 1) * sizeof(SphereRec);
        MIGCK(hipMalloc(&newOGid, std::max<size_t>(nONew, 1) * 4));
        MIGCK(hipMalloc(&newSGid, std::max<size_t>(nSNew, 1) * 4));
        OwnerRec* no = newOwners.as<OwnerRec>();
        SphereRec* ns_ = newSpheres.as<SphereRec>();
        DevBuf newOW[8], newGW[8];  // the wildcard arrays of the re-assembled slab
        MigWcPtrs nOWp{}, nGWp{};
        for (uint32_t k = 0; k < w.nOW; k++) {
            MIGCK(hipMalloc(&newOW[k].p, std::max<size_t>(nONew, 1) * 4));
            newOW[k].bytes = std::max<size_t>(nONew, 1) * 4, nOWp.p[k] = newOW[k].as<float>();
            if (w.nOwnNew)
                MIGCK(hipMemcpyAsync(newOW[k].p, w.ownOW.p[k], (size_t)w.nOwnNew * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        for (uint32_t k = 0; k < w.nGW; k++) {
            MIGCK(hipMalloc(&newGW[k].p, std::max<size_t>(nSNew, 1) * 4));
            newGW[k].bytes = std::max<size_t>(nSNew, 1) * 4, nGWp.p[k] = newGW[k].as<float>();
            if (w.sOwnNew)
                MIGCK(hipMemcpyAsync(newGW[k].p, w.ownGW.p[k], (size_t)w.sOwnNew * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        if (w.nOwnNew) {
            MIGCK(hipMemcpyAsync(no, w.ownOwners, (size_t)w.nOwnNew * sizeof(OwnerRec), hipMemcpyDeviceToDevice, c->stream));
            MIGCK(hipMemcpyAsync(newOGid, w.ownGid, (size_t)w.nOwnNew * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        if (w.sOwnNew) {
            MIGCK(hipMemcpyAsync(ns_, w.ownSpheres, (size_t)w.sOwnNew * sizeof(SphereRec), hipMemcpyDeviceToDevice, c->stream));
            MIGCK(hipMemcpyAsync(newSGid, w.ownSGid, (size_t)w.sOwnNew * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        uint32_t ob = w.nOwnNew, sb = w.sOwnNew;
        for (int k = 0; k < 2; k++) {
            const MigBuf& b = w.grecv[k];
            if (b.nC) {
                uint32_t* nsp = (uint32_t*)w.mem.alloc(((size_t)b.nC + 1) * 4);
                uint32_t* off = (uint32_t*)w.mem.alloc(((size_t)b.nC + 1) * 4);
                if (!nsp || !off)
                    return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
                hipLaunchKernelGGL(k_mig_nsph, dim3(grid_for((size_t)b.nC + 1)), dim3(256), 0, c->stream, b.nC, (const MigClump*)b.clumps, nsp);
                if (int rc = mig_scan_u32(g, c, nsp, off, (size_t)b.nC + 1))
                    return rc;
                hipLaunchKernelGGL(k_mig_unpack, dim3(grid_for(b.nC)), dim3(256), 0, c->stream, b.nC, (const MigClump*)b.clumps,
                                   (const MigSphere*)b.spheres, off, ob, sb,
                                   (uint32_t)(OWNER_GHOST_BIT | ((k == 0 && g->pairsOnce) ? OWNER_PASSIVE_BIT : 0u)), no, ns_, (uint32_t*)newOGid,
                                   (uint32_t*)newSGid);
                if (w.nOW || w.nGW)
                    hipLaunchKernelGGL(k_mig_unpack_wc, dim3(grid_for(b.nC)), dim3(256), 0, c->stream, b.nC, (const float*)b.owc, (const float*)b.swc, off,
                                       ob, sb, w.nOW, w.nGW, nOWp, nGWp);
            }
            ob += b.nC, sb += b.nS;
        }
        if (w.nX)
            hipLaunchKernelGGL(k_mig_copy_extras, dim3(grid_for(w.nX)), dim3(256), 0, c->stream, w.nX, c->owners.as<OwnerRec>(),
                               (const uint32_t*)q.ownerGid, w.nClumps, nClNew, no, (uint32_t*)newOGid);
        if (w.nX && w.nOW)  // (a replicated owner's wildcards stay this slab's own)
            hipLaunchKernelGGL(k_mig_copy_extras_wc, dim3(grid_for(w.nX)), dim3(256), 0, c->stream, w.nX, w.nClumps, nClNew, w.nOW, w.oldOW, nOWp);
        const int shift = (int)nClNew - (int)w.nClumps;
        if (shift && c->nAnal)
            hipLaunchKernelGGL(k_mig_shift_anal, dim3(grid_for(c->nAnal)), dim3(256), 0, c->stream, c->nAnal, c->anal.as<AnalObj>(), shift);
        if (shift && c->nTri)
            hipLaunchKernelGGL(k_mig_shift_tris, dim3(grid_for(c->nTri)), dim3(256), 0, c->stream, c->nTri, c->tris.as<uint32_t>(), shift);
        // ---- history: candidates = own rows, rows from the left, rows from the right
        const uint32_t nWs = std::max(w.nW, 1u);
        const uint32_t nCand = (uint32_t)w.nC + w.recv[0].nR + w.recv[1].nR;
        uint64_t nSeed = 0;
        uint64_t* seedKeys = nullptr;
        float* seedWc = nullptr;
        uint8_t* seedMark = nullptr;
        const bool anyPersist = g->anyPersist;  // (agreed on by the group: a neighbour's rows may carry marks this slab has none of)
        if (nCand) {
            MigRowHead* ch = (MigRowHead*)w.mem.alloc((size_t)nCand * sizeof(MigRowHead));
            float* cw = (float*)w.mem.alloc((size_t)nCand * nWs * 4);
            uint32_t *sk = (uint32_t*)w.mem.alloc((size_t)std::max(nSNew, 1u) * 4), *sv = (uint32_t*)w.mem.alloc((size_t)std::max(nSNew, 1u) * 4);
            uint32_t *sk2 = (uint32_t*)w.mem.alloc((size_t)std::max(nSNew, 1u) * 4), *sv2 = (uint32_t*)w.mem.alloc((size_t)std::max(nSNew, 1u) * 4);
            uint64_t *k0 = (uint64_t*)w.mem.alloc((size_t)nCand * 8), *k1 = (uint64_t*)w.mem.alloc((size_t)nCand * 8);
            uint32_t *r0 = (uint32_t*)w.mem.alloc((size_t)nCand * 4), *r1 = (uint32_t*)w.mem.alloc((size_t)nCand * 4);
            uint32_t *keep = (uint32_t*)w.mem.alloc(((size_t)nCand + 1) * 4), *kpos = (uint32_t*)w.mem.alloc(((size_t)nCand + 1) * 4);
            seedKeys = (uint64_t*)w.mem.alloc((size_t)nCand * 8);
            seedWc = (float*)w.mem.alloc((size_t)nCand * nWs * 4);
            seedMark = anyPersist ? (uint8_t*)w.mem.alloc((size_t)nCand) : nullptr;
            if ((anyPersist && !seedMark) || !ch || !cw || !sk || !sv || !sk2 || !sv2 || !k0 || !k1 || !r0 || !r1 || !keep || !kpos || !seedKeys || !seedWc)
                return gfail(g, DEME_ERR_HIP, "migrate: out of device memory");
            size_t at = 0;
            auto append = [&](const void* h, const void* wv, size_t n) -> int {
                if (!n)
                    return DEME_OK;
                MIGCK(hipMemcpyAsync(ch + at, h, n * sizeof(MigRowHead), hipMemcpyDeviceToDevice, c->stream));
                if (w.nW)
                    MIGCK(hipMemcpyAsync(cw + at * nWs, wv, n * nWs * 4, hipMemcpyDeviceToDevice, c->stream));
                at += n;
                return DEME_OK;
            };
            if (int rc = append(w.rowH, w.rowW, (size_t)w.nC))
                return rc;
            if (int rc = append(w.recv[0].rowH, w.recv[0].rowW, w.recv[0].nR))
                return rc;
            if (int rc = append(w.recv[1].rowH, w.recv[1].rowW, w.recv[1].nR))
                return rc;
            // global -> local sphere ids of the re-assembled slab
            hipLaunchKernelGGL(k_mig_iota_gid, dim3(grid_for(std::max(nSNew, 1u))), dim3(256), 0, c->stream, nSNew, (const uint32_t*)newSGid, sk, sv);
            if (nSNew)
                if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
                        return rocprim::radix_sort_pairs(tmp, bytes, sk, sk2, sv, sv2, (size_t)nSNew, 0, 32, c->stream);
                    }))
                    return gfail(g, rc, "migrate: %s", c->err.c_str());
            hipLaunchKernelGGL(k_mig_localise, dim3(grid_for(nCand)), dim3(256), 0, c->stream, nCand, w.nW, q.flipMask, ch, cw, sk2, sv2, nSNew, ns_,
                               w.nOwnNew, k0, r0);
            if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
                    return rocprim::radix_sort_pairs(tmp, bytes, k0, k1, r0, r1, (size_t)nCand, 0, 64, c->stream);
                }))
                return gfail(g, rc, "migrate: %s", c->err.c_str());
            hipLaunchKernelGGL(k_mig_keep_flags, dim3(grid_for((size_t)nCand + 1)), dim3(256), 0, c->stream, nCand, k1, keep);
            if (int rc = mig_scan_u32(g, c, keep, kpos, (size_t)nCand + 1))
                return rc;
            uint32_t nKeep = 0;
            GHIP(hipMemcpyAsync(&nKeep, kpos + nCand, 4, hipMemcpyDeviceToHost, c->stream));
            hipLaunchKernelGGL(k_mig_seed, dim3(grid_for(nCand)), dim3(256), 0, c->stream, nCand, w.nW, k1, r1, keep, kpos, cw, seedKeys, seedWc,
                               (const MigRowHead*)ch, seedMark);
            GHIP(hipStreamSynchronize(c->stream));
            nSeed = nKeep;
        }
        GHIP(hipStreamSynchronize(c->stream));
        // ---- install
        hipFree(c->owners.p);
        hipFree(c->spheres.p);
        c->owners = newOwners, c->spheres = newSpheres;
        for (uint32_t k = 0; k < w.nOW; k++) {
            if (c->userWc[0][k].p)
                hipFree(c->userWc[0][k].p);
            c->userWc[0][k] = newOW[k];
        }
        for (uint32_t k = 0; k < w.nGW; k++) {
            if (c->userWc[1][k].p)
                hipFree(c->userWc[1][k].p);
            c->userWc[1][k] = newGW[k];
        }
        hipFree(q.ownerGid);
        hipFree(q.sphereGid);
        q.ownerGid = newOGid, q.sphereGid = newSGid;
        q.nOwn = w.nOwnNew, q.nGL = nGL, q.nGR = nGR;
        c->nOwners = nONew, c->nOwnerClumps = nClNew, c->nSpheres = nSNew;
        c->hasGhosts = (nGL + nGR) > 0;
        c->dp.hasGhosts = c->hasGhosts ? 1u : 0u;
        refresh_dev_params(c);
        if (int rc = mig_scratch_for_counts(c, nONew, nSNew))
            return gfail(g, rc, "migrate: %s", c->err.c_str());
        if (nSeed > c->cntCap)
            if (int rc = grow_contact_arena(c, (size_t)nSeed + nSeed / 4 + 1024))
                return gfail(g, rc, "migrate: %s", c->err.c_str());
        if (nSeed) {
            MIGCK(hipMemcpyAsync(c->keysSorted[c->keysCur].p, seedKeys, (size_t)nSeed * 8, hipMemcpyDeviceToDevice, c->stream));
            if (w.nW)
                MIGCK(hipMemcpyAsync(c->wc[c->wcCur].p, seedWc, (size_t)nSeed * w.nW * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        c->nContacts = nSeed, c->nPrev = 0, c->nWcStored = nSeed;
        c->listSerial++;
        // the marked contacts of the re-assembled slab (the rows carried the marks; a pair both neighbours knew arrived twice, alike)
        c->hPersist.clear();
        if (anyPersist && nSeed) {
            std::vector<uint8_t> hm(nSeed);
            std::vector<uint64_t> hk(nSeed);
            MIGCK(hipMemcpyAsync(hm.data(), seedMark, (size_t)nSeed, hipMemcpyDeviceToHost, c->stream));
            MIGCK(hipMemcpyAsync(hk.data(), seedKeys, (size_t)nSeed * 8, hipMemcpyDeviceToHost, c->stream));
            GHIP(hipStreamSynchronize(c->stream));
            for (size_t i = 0; i < nSeed; i++)
                if (hm[i])
                    c->hPersist.push_back(hk[i]);  // (ascending: the seeds are sorted)
            if (!c->hPersist.empty()) {
                if (ensure(c, c->persistKeys, c->hPersist.size() * 8))
                    return gfail(g, c->lastStatus, "migrate: %s", c->err.c_str());
                MIGCK(hipMemcpyAsync(c->persistKeys.p, c->hPersist.data(), c->hPersist.size() * 8, hipMemcpyHostToDevice, c->stream));
            }
        }
        // replicated free owners keep their place behind the clumps: their numbers move with the clump count
        if (!c->hShared.empty() && shift) {
            for (auto& o : c->hShared)
                o = (uint32_t)((int)o + shift);
            MIGCK(hipMemcpyAsync(c->sharedIds.p, c->hShared.data(), c->hShared.size() * 4, hipMemcpyHostToDevice, c->stream));
        }
        c->haveList = true, c->seeded = true, c->mapFresh = false, c->conValid = false, c->listStale = false;
        c->list[c->cur].invalidate();
        c->conTile = false;
        c->prescDirty = true;
        // per-owner records of the slab as it was do not carry over (as in deme_upload_scene; not clear_next_acc, which zeroes the
        // records of the same owners after their step): without its host mirror the device copy is not read before the next
        // deme_add_owner_acc, which sizes and zeroes both for the new owner count
        c->nextAccPending = false;
        c->hNextAcc.clear();
        // ---- exchange lists: what I receive sits in the two ghost sections, what I send is what I packed
        for (int k = 0; k < 2; k++) {
            HaloSide& sd = sl.side[k];
            for (void* p : {sd.sendIds, sd.recvIds, sd.sendBuf, sd.recvBuf})
                if (p)
                    hipFree(p);
            sd.sendIds = sd.recvIds = sd.sendBuf = sd.recvBuf = nullptr;
            g->bytesPerStep -= (uint64_t)sd.nSend * sizeof(GhostRec);
            sd.nSend = sd.nRecv = 0;
            if (sd.peerRank < 0)
                continue;
            sd.nSend = w.gsend[k].nC, sd.nRecv = k ? nGR : nGL;
            MIGCK(hipMalloc(&sd.sendIds, std::max<size_t>(sd.nSend, 1) * 4));
            MIGCK(hipMalloc(&sd.recvIds, std::max<size_t>(sd.nRecv, 1) * 4));
            MIGCK(hipMalloc(&sd.sendBuf, std::max<size_t>(sd.nSend, 1) * sizeof(GhostRec)));
            MIGCK(hipMalloc(&sd.recvBuf, std::max<size_t>(sd.nRecv, 1) * sizeof(GhostRec)));
            if (sd.nSend)
                MIGCK(hipMemcpyAsync(sd.sendIds, w.sendIds[k], (size_t)sd.nSend * 4, hipMemcpyDeviceToDevice, c->stream));
            if (sd.nRecv)
                hipLaunchKernelGGL(k_mig_iota, dim3(grid_for(sd.nRecv)), dim3(256), 0, c->stream, sd.nRecv, w.nOwnNew + (k ? nGL : 0u),
                                   (uint32_t*)sd.recvIds);
            g->bytesPerStep += (uint64_t)sd.nSend * sizeof(GhostRec);
        }
        sl.nOwnersAtAttach = c->nOwners;  // (the exchange lists were just rebuilt for the re-assembled slab)
        if (int rc = rev_setup_slab(g, sl))
            return rc;
        GHIP(hipStreamSynchronize(c->stream));
        if (c->evStepDone)
            GHIP(hipEventRecord(c->evStepDone, c->stream));
        if (g->nOwnersGlobal && getenv("DEME_MIG_CHECK")) {  // self-check: every id of the re-assembled slab names a row of the global scene
            std::vector<uint32_t> hg(c->nOwners);
            GHIP(hipMemcpy(hg.data(), q.ownerGid, (size_t)c->nOwners * 4, hipMemcpyDeviceToHost));
            for (uint32_t o = 0; o < c->nOwners; o++)
                if (hg[o] >= g->nOwnersGlobal)
                    return gfail(g, DEME_ERR_INVALID, "migrate check: slab %zu slot %u (own %u, ghosts %u + %u, extras %u) holds id %u of %u", i, o,
                                 w.nOwnNew, nGL, nGR, w.nX, hg[o], g->nOwnersGlobal);
        }
    }
    if (clumpsMoved)
        *clumpsMoved = moved;
    return DEME_OK;
}
