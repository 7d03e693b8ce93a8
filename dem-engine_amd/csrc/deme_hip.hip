// deme_hip.hip -- host orchestration (C++) and the C-ABI of include/deme_hip.h.
//
// One context = one GPU = one HIP stream.  The reference splits this work between a kinematic
// thread (DEM/kT.cpp) and a dynamic thread (DEM/dT.cpp) that exchange device buffers under mutexes;
// here contact detection and stepping are phases on the same stream, sized through two small
// device->host reads per detection (the reference makes >=10, DEMCubContactDetection.cu:121-905).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <dlfcn.h>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
// Radix-sort configurations measured on MI355X for the detection's list sizes (a few million entries: the library's defaults are
// tuned for lists that fill the chip many times over; at these sizes workgroups of 1024 with 8 keys each shorten the chained
// look-back of every pass).  tools/rsbench.hip, profiles/r04/r04j_radix_configs.txt: incidences (8.2e6 pairs, 21 bits) 227 -> 206 us (4.4e6: 192 -> 149),
// crossing records by B owner (1.4e6 pairs, 20 bits, two 10-bit passes) 108 -> 68 us, contact keys (4.3e6 u64, 24 bits) 150 -> 141 us.
template <unsigned RB, unsigned IPT = 8>
using DemeRadixCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                                rocprim::radix_sort_onesweep_config<rocprim::kernel_config<1024, IPT>, rocprim::kernel_config<1024, IPT>, RB,
                                                                                    rocprim::block_radix_rank_algorithm::match>,
                                                1024 * 1024>;
#include <array>
#include <iterator>
#include <limits>

#include "../../include/deme_hip.h"
#include "deme_device.h"
#include "deme_force.h"
#include "deme_force_fast.h"
#include "deme_jit.h"
#include "deme_kernels.h"
#include "deme_tile.h"
#include "deme_tile_step.h"
#include "deme_migrate.h"
#include "deme_mesh_kernels.h"
#include "deme_resize.h"
#include "deme_query.h"
#include "deme_contact_inspect.h"
#include "deme_tri_loads.h"
#include "deme_tri_wear.h"
#include "deme_fields.h"
#include "deme_clusters.h"
#include "deme_sort.h"

using namespace deme_dev;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// the (key, value) pairs of one user of the segmented sum (seg_reserve, seg_sort, seg_sums): [0] as selected, [1] sorted
struct SegPairs {
    DevBuf key[2], val[2];
};

// One built contact list: what a detection's part 2 (detect_part2, build_legacy_lists) writes and the stepping kernels read, with
// the host scalars that describe it.  A context holds two (deme_ctx::list): an asynchronous detection builds one while the steps
// in flight read the other, and the pair is swapped by flipping an index.  Everything else a list refers to is shared by both
// and stays on the context -- see the note at deme_ctx::list.
struct ContactList {
    // per contact (size_list_per_contact)
    DevBuf mapping, ownerA, ownerB[2], bIdx[2], info, tInfo, rIdx, lPos, remVal, rankC, remKey[2], cDefer, blockMode, smFlag, smList;
    // per owner / per tile (size_list_per_owner)
    DevBuf aStart, bStart, heavy, fixedFlag, heavyList, rangeCtr, hList, hCount, tileMode, tileOrg, rStart, lOff, lCount, tileRem, tileBase,
        tileBig, bigList;
    uint64_t nListed = 0;      // contacts the owner arrays (ownerA, ownerB[0], info ...) were built for
    int listKeys = 0;          // ... and the key buffer (deme_ctx::keysSorted) they were built from
    bool legacyLists = false;  // the B-sorted list of the round-2 kernels exists (built on demand when the list has tile structures)
    bool tileActive = false;   // the list has tile structures (built-in model, fast mode, every halo fits)
    bool fusedList = false;    // the list has the incoming structures of the one-kernel step (decided per detection)
    bool fusedChecked = false;  // ... and the device has been asked whether every closed tile fits
    // the heavy-owner counts of a tiled list are fetched without stopping the stream: the copy lands in pinned memory
    // (the PIN_HEAVY slot of deme_ctx::pin), the first reader (launch_reduce_heavy, one force launch later) waits for its event
    bool hrPending = false, heavyOverflow = false;
    uint32_t nHeavy = 0, nHeavyFree = 0, nSA = 0, nSM = 0;
    uint32_t nBigTiles = 0, tileMaxHalo = 0, tileMaxList = 0, tileMaxHaloIn = 0;

    // nothing is built: whatever changes the owners, their slots or the keys under a list calls this, and the detection that
    // always follows describes the list again
    void invalidate() {
        nListed = 0, listKeys = 0;
        legacyLists = tileActive = fusedList = fusedChecked = hrPending = heavyOverflow = false;
        nHeavy = nHeavyFree = nSA = nSM = 0;
        nBigTiles = tileMaxHalo = tileMaxList = tileMaxHaloIn = 0;
    }
    std::array<DevBuf*, 35> buffers() {
        return {&mapping, &ownerA, &ownerB[0], &ownerB[1], &bIdx[0], &bIdx[1], &info, &tInfo, &rIdx, &lPos, &remVal, &rankC, &remKey[0],
                &remKey[1], &cDefer, &blockMode, &smFlag, &smList, &aStart, &bStart, &heavy, &fixedFlag, &heavyList, &rangeCtr, &hList,
                &hCount, &tileMode, &tileOrg, &rStart, &lOff, &lCount, &tileRem, &tileBase, &tileBig, &bigList};
    }
};

struct TimerSlot {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0;
    uint64_t launches = 0;
    uint64_t seen = 0;  // launches since the last reset, timed or not
};

}  // namespace

struct deme_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = true;
    std::string err;
    DemeParams hp{};
    bool haveParams = false, haveScene = false;
    DevParams dp{};
    uint32_t nOwners = 0, nOwnerClumps = 0, nSpheres = 0, nAnal = 0, nMat = 0, nComp = 0, nMassProps = 0;
    // model
    DevBuf owners, spheres, acc, comp, massProps, anal, matPair, E, nu, CoR, mu, Crr, famMasks, famExtra, famFlags;
    std::vector<uint8_t> hObjType;  // host copy for contact-type decoding on download
    // the component table as the device holds it (deme_change_owner_sizes derives entries from it); the first nTemplateComps
    // entries are the uploaded scene's and always stay, the others are derived by resizes and dropped when no sphere uses them
    std::vector<float4> hComp;
    uint32_t nTemplateComps = 0;
    DevBuf rsMark, rsKeys[2], rsRuns, rsUKeys, rsIdx, rsOldR, rsUses, rsRemap;  // resize scratch (deme_resize.h), allocated by the first resize
    // owner-filtered contact queries (deme_query.h): marks per owner, the hit rows and their records, the hit counter; allocated by
    // the first query and kept, so that a script asking every frame selects once per call
    DevBuf qMark, qHits, qRecs, qCtr, qState;  // (qState: the owner records deme_query_owner_state gathers)
    uint64_t qHostBytes = 0;  // bytes the queries have copied to the host so far (deme_query_host_bytes)
    // contact inspectors (deme_contact_inspect.h): the mask and the side counts per owner slot, the blocks' partials with the result
    // behind them, the counts in the caller's (or global) ids; allocated by the first call and kept
    DevBuf ciMask, ciCounts, ciPartial, ciOut;
    // the segmented sums of the inspectors below (deme_seg_sum.h): the sort's own scratch (never the detection's: an asynchronous
    // detection may be sorting) and the blocks' partials.  One pair for all of them: every inspector pass is enqueued on the
    // context's own stream, so no two are in flight at once.  Kept likewise
    DevBuf segTmp, segPartial;
    // triangle loads (deme_tri_loads.h): the (triangle, row) pairs before and after the sort, the sums and counts per triangle
    SegPairs tlPairs;
    DevBuf tlForce, tlCount;
    // mesh wear (deme_tri_wear.h): six doubles and one uint64_t count per triangle, summed from sample to sample on the device; the
    // pairs of a sample are tlPairs (the same select on the same stream).  twTri: the triangles the arrays were cleared for
    bool twOn = false;
    DevBuf twAcc, twRows, twOut;  // (twOut: the asked columns packed for deme_tri_wear_read)
    uint32_t twTri = 0;
    double twTime = 0;  // the sum of the weights of the samples taken
    // field inspector (deme_fields.h): the cell of every owner slot, the (cell, slot) and (cell, side) pairs before and after their
    // sorts, the columns of every cell
    SegPairs fiOwn, fiSide;
    DevBuf fiCellOf, fiOut;
    // cluster inspector (deme_clusters.h): parent, label, size, row flag and rank per caller id, the (label, slot) pairs before and
    // after their sort, the integer partials with the summary behind them, the table, the control words, a slab's (global id, global
    // root) pairs
    SegPairs clSel;
    DevBuf clParent, clLabel, clSize, clFlag, clRank, clStat, clTable, clCtl, clPairs;
    uint32_t clRetries = 0;  // compare-and-swaps the last call's link pass lost (deme_clusters_link_retries)
    std::map<std::string, int> regionBySource;  // deme_multi_inspect_contacts: a region string compiles once per slab context
    // detection scratch
    DevBuf sphFam;  // per sphere: its owner's family word, for the sweeps (written by k_sphere_prep when masks, margins or ghosts are in play)
    DevBuf geo, binLo, binN, binPartial, incKeys[2], incVals[2], keysRaw, keysMid, keysSorted[2], wc[2], ctr,
        scanTmp, sortTmp, rec[4], stage;
    // The contact list the steps read (list[cur]) and the one an asynchronous detection builds beside them (list[cur ^ 1]).
    // Shared by both, on purpose: the key and history double buffers with their selectors (keysSorted, wc, keysCur, wcCur ...),
    // the per-contact products of the force pass (conA*, conB*, aSum, rec32, rec[]), the pinned target of the heavy-owner
    // read-back (the PIN_HEAVY slot, hrEvent) and the closed-tile structures of the one-kernel step (recContact, inCnt ... below).
    ContactList list[2];
    int cur = 0;
    // per-contact contributions of the force pass
    DevBuf conA4, conA2, conB4, conB2, aSum, rec32;
    // One pinned slot and one event serve the pending read-back (ContactList::hrPending) of both lists: a list's read-back is
    // resolved by the first force launch on it, or superseded when the list is built again, before the other list's is issued
    // -- an asynchronous cycle enqueues D >= 1 steps on the current list before part 2 builds the other.
    hipEvent_t hrEvent = nullptr;
    bool ctrFresh = false;  // DetectCounters were zeroed by the margins kernel's launch and nothing has counted in them since
    bool conTile = false;     // the contributions in memory were written by the tile kernel
    // the whole step in one kernel (deme_tile_step.h): closed tiles -- a contact that straddles two tiles is evaluated by both --
    // integrate their own owners; owners and history are double-buffered
#define DEME_FUSED_AUTO_MAX_OWNERS 100000u  // deme_set_fused_step(ctx, 2): the one-kernel step where it was measured faster (header)
    int fusedEnable = 0;          // deme_set_fused_step / DEME_FUSED=1: the one-kernel step (measured slower on the packed bed: DESIGN 3.7)
    bool fusedPrevValid = false;  // the last step was a fused one: the buffers of its start are intact (a / alpha can be replayed from them)
    uint64_t nFusedSteps = 0;
    // (these exist once, not per list: only k_tile_incoming and k_tile_step read them, and the one-kernel step is never chosen for
    // a list built while asyncLead != 0.  k_tile_build writes recContact unconditionally, so the pointer is always valid -- also
    // when part 2 runs on the detection stream, where nothing in flight reads it.)
    DevBuf ownersNext, recContact, inCnt, inStart, tInfoIn, inContact, hCountIn;
    // A run-time compiled model takes the tile pass only when a tile holds enough contacts to pay for its staging (measured on
    // configs[4], 1e6 single spheres with 1.6 contacts each = 200 per tile: tile pass 0.058 ms against 0.044 ms for the general
    // kernel; at the 555 per tile of three-sphere clumps the tile pass wins as it does for the built-in models).
    uint32_t tileMinContactsCustom = 320;
    uint64_t lastSegMax = 0;             // longest segment of the last detection (sizes the early launch of k_compact_keys)
    size_t keySegMin = (size_t)1 << 20;  // arenas from this many slots on are cut into DEME_KEY_SEGS segments (DEME_KEY_SEG_MIN; 0: never)
    // persistent contacts: the sorted set of marked keys (host copy + device copy appended to every detection's raw keys)
    DevBuf persistKeys, binStat;
    // acceleration the script adds for the next step only (deme_add_owner_acc): device records + host mirror
    DevBuf nextAcc;
    std::vector<AccRec> hNextAcc;
    bool nextAccPending = false;
    std::vector<uint64_t> hPersist;
    // triangles (mesh path)
    uint32_t nTri = 0;
    DevBuf tris, triWorld, triLo, triHi, triCounts, triOffsets, triKeys[2], triVals[2];
    size_t triCap = 0;
    uint64_t nTriInc = 0;
    // run-time compiled user force model
    deme_jit::MaterialTables mt;
    hipModule_t customMod = nullptr;
    hipFunction_t customFn[3] = {nullptr, nullptr, nullptr};
    hipFunction_t customTileFn[4] = {nullptr, nullptr, nullptr, nullptr};  // the tile pass with the user's model (deme_jit::kTileEntry)
    std::map<size_t, std::vector<char>> jitCache;
    bool conValid = false;
    int keysCur = 0, wcCur = 0;
    size_t incCap = 0, cntCap = 0;
    uint64_t nInc = 0, nContacts = 0, nPrev = 0, nWcStored = 0;
    uint64_t nActiveBins = 0;
    uint32_t maxInBin = 0;
    bool haveList = false, mapFresh = false;
    bool seeded = false;
    // family motion prescriptions: run-time compiled kernel + the owners it applies to
    hipModule_t prescMod = nullptr;
    hipFunction_t prescFn = nullptr;
    DevBuf prescList, prescSlot, prescRec;
    DevBuf userWc[4][8];  // [kind: owners, spheres, triangles, analytical][index]
    uint32_t nOwnerWc = 0, nGeoWc = 0;
    bool hasGhosts = false;  // a family carries DEME_FAMILY_GHOST: force passes can be split for the halo overlap
    // asynchronous detection (deme_set_async_detection): part 1 of a detection on its own stream, from a snapshot of the owners,
    // `asyncLead` steps before the list it builds is swapped in
    uint32_t asyncLead = 0;
    // (slab group) one evaluation per cross-cut contact: where an own clump finds the a / alpha the left neighbour evaluated for it
    DevBuf revSlot;
    const void* revAcc = nullptr;
    bool pairsOnce = false;
    PrescArgs laterPa{nullptr, nullptr};  // the prescription records of the step whose integration is split (launch_integrate_later)
    bool crossStale = false;  // a scene was uploaded while the group evaluates cross-cut contacts once: rev_setup_slab runs again first
    char* pin = nullptr;       // 16 KB of pinned host memory: where the detection's read-backs land
    int spinSync = 1;          // DEME_SPIN_SYNC=0: blocking waits at the detection's read-backs
    bool snapPending = false;  // (slab group) take the owner snapshot of an asynchronous detection in this step, once the ghosts are in place
    DevBuf ownersSnap;
    hipStream_t detStream = nullptr;
    hipEvent_t evSnap = nullptr, evP1 = nullptr;
    uint64_t nAsyncDetections = 0;
    std::vector<uint32_t> hShared;  // replicated free owners (DemeScene.ownerGhost bit 1): their a / alpha are summed across slabs
    DevBuf sharedIds, sharedBuf;
    bool tailFused = true;
    bool inGroupStep = false;
    hipStream_t haloStream = nullptr;
    hipEvent_t evStepDone = nullptr, evHaloDone = nullptr;
    bool overlapDetect = false;  // the step opened by deme_step_overlap_begin needs a detection first
    hipModule_t rulesMod = nullptr;
    // adaptive controllers (deme_set_adaptive)
    DemeAdaptive ad{};
    hipEvent_t evDet0 = nullptr, evDet1 = nullptr, evWin0 = nullptr, evWin1 = nullptr;
    double binAccMs = 0, binPrevMs = -1, freqPrevMs = -1;
    float binRate = 0.f;
    uint32_t binObs = 0, freqObs = 0, nBinChanges = 0, nFreqChanges = 0;
    uint64_t winStartStep = 0;
    int freqDir = 1, binFlip = 1;
    bool winOpen = false;
    // inspector region filters: one module per compiled region (id = index)
    std::vector<hipModule_t> regionMod;
    std::vector<hipFunction_t> regionFn;
    DevBuf volumes;  // per mass-property entry: declared clump volume ("clump_volume" inspector)
    bool haveVolumes = false;
    hipFunction_t rulesFn = nullptr;  // on-the-fly family changes
    bool rulesNeedAcc = false;
    uint32_t nPresc = 0;
    uint8_t hostFamFlags[DEME_NUM_FAMILIES] = {0};
    bool prescDirty = true;  // owner -> family assignment changed: rebuild the list  // the list was loaded by deme_seed_contacts: it only feeds the next history map
    bool record = false;
    uint64_t nSteps = 0, nDetections = 0;
    uint32_t stepsSinceCD = 0;
    // the script moved a body, changed a family or rewrote triangle nodes: the K-step list and its margins no longer cover the
    // scene, so the next step starts with a detection (the reference: pendingCriticalUpdate / stampLastDynamicUpdateProdDate = -1,
    // DEM/dT.cpp:2351)
    bool listStale = false;
    uint32_t lastStatus = 0;
    double timeElapsed = 0;
    // arithmetic mode (deme_set_arith_mode): DEME_ARITH_FAST (default) or DEME_ARITH_EXACT
    int arith = DEME_ARITH_FAST;
    uint32_t xcdGroup = 0;  // XCD-aware block order of the force kernel (ForceArgs::xcdGroup)
    // engine-side spatial order (deme_order.inc): slot -> caller id and back, for owners and spheres (empty: the caller's order)
    bool permuted = false;
    int reorderEnable = 1;
    std::vector<uint32_t> hO2E, hE2O, hS2E, hE2S;
    DevBuf dO2E, dS2E;
    double orderSpread[2] = {0, 0};  // cells per tile bounding box: in the caller's order, along the curve
    // renewing the order at run time (order_renew): the engine watches the tiles of every detection -- mean foreign owners per
    // tile, tiles that no longer fit -- against what they were right after the last (re)ordering
    bool orderEligible = false;     // the scene may be reordered (fast mode, no ghosts: what order_decide checks)
    bool orderStructOK = false;     // ... the part of that which does not depend on the arithmetic mode
    bool geoStale = false;          // the per-sphere geometry of the last detection sits in slots an order renewal has left
    bool orderRenewDue = false;
    uint32_t orderBaseHalo = 0;     // mean halo (x 16) at the first detection after the last ordering; 0 = not taken yet
    uint64_t orderDetAt = 0, nOrderRenewals = 0;
    uint64_t listSerial = 0, viewSerial = ~0ull;  // the caller's view of the current list (ids and order), cached per list
    std::vector<uint64_t> viewKeys;
    std::vector<uint32_t> viewPerm;
    int timing = 0;  // 0 off; n > 0: every n-th launch of each timed kernel is bracketed with HIP events
    std::map<std::string, TimerSlot> timers;
    std::vector<hipEvent_t> eventPool;
};

namespace {

int fail(deme_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) {
        c->err = buf;
        c->lastStatus = (uint32_t)code;
    }
    return code;
}

// the class field of a contact key for a contact type of the C-ABI (every analytical type is one class)
inline uint64_t key_class_of_type(uint8_t type) {
    return type == DEME_SPHERE_SPHERE_CONTACT ? DEME_KEY_CLASS_SS : type == DEME_SPHERE_MESH_CONTACT ? DEME_KEY_CLASS_SM : DEME_KEY_CLASS_SA;
}

// What every reader of the contact records (deme_download_contact_records, the by-owner query with records, the contact inspectors,
// and their forms of a decomposed run, slab by slab) refuses of a list without them: the code, with the text left in c->err.
int records_refused(deme_ctx* c) {
    if (!c->record)
        return fail(c, DEME_ERR_INVALID, "contact recording is off (deme_set_record_contacts)");
    if (c->seeded)
        return fail(c, DEME_ERR_INVALID, "the list is a seed (deme_seed_contacts, or the engine's order was just renewed): its contacts have not been evaluated yet -- step or detect first");
    return DEME_OK;
}

#define HIPCK(call)                                                                                   \
    do {                                                                                              \
        hipError_t _e = (call);                                                                       \
        if (_e != hipSuccess)                                                                         \
            return fail(c, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// The sizing read-backs of a detection: the host has nothing else to do, the GPU idles until it is back with the next launches,
// and a blocking wait wakes up tens of microseconds late -- so the host polls the stream (for at most a few milliseconds; a
// part 1 beside the steps, whose wait is long by design, blocks instead of burning a core).
// They land in the context's pinned block (a copy into pageable memory goes through the runtime's staging buffer and costs tens
// of microseconds of host time before the wait even starts), each in a slot of its own where two can be in flight at the same
// time: part 1 on the detection stream beside ensure_legacy_lists on the main stream, and the heavy-owner counts of a tiled
// list (ContactList::hrPending), which nobody waits for until the next force launch.
constexpr size_t PIN_BYTES = 16384;
constexpr size_t PIN_HEAVY = 0;      // RangeCounters: the pending heavy-owner counts
constexpr size_t PIN_RANGES = 128;   // RangeCounters: part 2's tile counters
constexpr size_t PIN_LEGACY = 256;   // RangeCounters: read_legacy_counts
constexpr size_t PIN_TRI = 384;      // uint32_t: the triangle incidences
constexpr size_t PIN_UNIQUE = 448;   // unsigned long long: the keys left once the marked contacts' duplicates are gone
constexpr size_t PIN_DETECT = 1024;  // DetectHead: part 1's counters (the incidence total is read through the same slot)
static_assert(PIN_HEAVY + sizeof(RangeCounters) <= PIN_RANGES && PIN_RANGES + sizeof(RangeCounters) <= PIN_LEGACY &&
                  PIN_LEGACY + sizeof(RangeCounters) <= PIN_TRI && PIN_TRI + sizeof(uint32_t) <= PIN_UNIQUE &&
                  PIN_UNIQUE + sizeof(unsigned long long) <= PIN_DETECT && PIN_DETECT + sizeof(DetectHead) <= PIN_BYTES,
              "the read-back slots overlap or leave the pinned block");
static_assert(PIN_RANGES % 8 == 0 && PIN_LEGACY % 8 == 0 && PIN_TRI % 8 == 0 && PIN_UNIQUE % 8 == 0 && PIN_DETECT % 8 == 0,
              "a read-back slot is aligned for the counters it holds");
template <typename T>
static inline T* pin_at(deme_ctx* c, size_t slot) {
    return reinterpret_cast<T*>(c->pin + slot);
}
static hipError_t sync_readback(deme_ctx* c, hipStream_t st, bool spin) {
    if (c->spinSync && spin) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int it = 0;; it++) {
            const hipError_t q = hipStreamQuery(st);
            if (q != hipErrorNotReady)
                return q;
            if ((it & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5))
                break;
        }
    }
    return hipStreamSynchronize(st);
}
// One read-back: `bytes` of device counters from `dev` into `slot`, ordered on `st`, and the wait for them.  nullptr: the copy or
// the wait failed (the error is in c->err, its code in c->lastStatus).
template <typename T>
const T* read_back(deme_ctx* c, size_t slot, const void* dev, hipStream_t st, bool spin, size_t bytes = sizeof(T)) {
    T* host = pin_at<T>(c, slot);
    hipError_t e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = sync_readback(c, st, spin);
    if (e == hipSuccess)
        return host;
    fail(c, DEME_ERR_HIP, "a detection's read-back failed: %s", hipGetErrorString(e));
    return nullptr;
}

int ensure(deme_ctx* c, DevBuf& b, size_t bytes, bool keep = false) {
    if (bytes <= b.bytes && b.p)
        return DEME_OK;
    size_t want = std::max<size_t>(bytes, 256);
    if (b.p)  // a buffer that grows once usually grows again (a settling bed: every detection a few more contacts): leave room
        want = std::max(want, b.bytes + b.bytes / 4);
    void* np = nullptr;
    HIPCK(hipMalloc(&np, want));
    if (keep && b.p && b.bytes)
        HIPCK(hipMemcpyAsync(np, b.p, b.bytes, hipMemcpyDeviceToDevice, c->stream));
    if (b.p) {
        HIPCK(hipStreamSynchronize(c->stream));
        HIPCK(hipFree(b.p));
    }
    b.p = np;
    b.bytes = want;
    return DEME_OK;
}

template <typename T>
int upload(deme_ctx* c, DevBuf& b, const T* src, size_t n) {
    int rc = ensure(c, b, std::max<size_t>(n, 1) * sizeof(T));
    if (rc)
        return rc;
    if (n && src)
        HIPCK(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    else if (n)
        HIPCK(hipMemsetAsync(b.p, 0, n * sizeof(T), c->stream));
    return DEME_OK;
}

// The two-call idiom of the rocprim device algorithms: size query, room in `tmp` (scanTmp or sortTmp), the call itself.
// call(void* storage, size_t& bytes) -> hipError_t
template <class Call>
int with_temp(deme_ctx* c, DevBuf& tmp, Call&& call) {
    size_t bytes = 0;
    HIPCK(call(nullptr, bytes));
    if (int rc = ensure(c, tmp, bytes))
        return rc;
    bytes = tmp.bytes;
    HIPCK(call(tmp.p, bytes));
    return DEME_OK;
}

// The detection's radix sorts: the project's own sort (deme_sort.h) from `ownFrom` entries on, rocprim with RocCfg below -- a pass
// of the own sort is three launches whatever n is, which a list of a few thousand entries does not earn back.  The thresholds
// are where tools/sortbench finds the two level on MI355X (profiles/r07/sort_ab.txt).  `cap`: the capacity of the arena the list
// lives in; the scratch is sized for it, so that a list growing inside its arena never makes a sort allocate.
// -DDEME_SORT_ROCPRIM=1 builds a library whose every site takes rocprim (A/B runs: make variant).
#ifndef DEME_SORT_ROCPRIM
#define DEME_SORT_ROCPRIM 0
#endif
// (each the smallest size measured at which the own sort is ahead, a tenth of which rocprim is; us, best of 9 -- at 82 000 pairs
// one repeat of nine was an outlier, the medians are 45 against 52)
constexpr size_t DEME_SORT_OWN_FROM_INCIDENCES = 82000;  // (bin, sphere) pairs, 21-22 key bits: 45 us against 51
constexpr size_t DEME_SORT_OWN_FROM_KEYS64 = 430000;     // contact keys, 24 key bits from bit 31: 48 us against 120
constexpr size_t DEME_SORT_OWN_FROM_RECORDS = 180000;    // crossing records by B owner, <= 20 key bits: 46 us against 60
inline bool sort_takes_own(size_t n, size_t cap, size_t ownFrom) {
    return !DEME_SORT_ROCPRIM && n >= ownFrom && std::max(n, cap) <= deme_sort::MAX_N;
}
template <class RocCfg, bool HAS_V, typename K>
hipError_t deme_radix_sort(void* tmp, size_t& bytes, const K* keysIn, K* keysOut, const uint32_t* valsIn, uint32_t* valsOut, size_t n, size_t cap,
                           unsigned beginBit, unsigned endBit, size_t ownFrom, hipStream_t st) {
    if (sort_takes_own(n, cap, ownFrom))
        return deme_sort::radix_sort<K, HAS_V>(tmp, bytes, keysIn, keysOut, valsIn, valsOut, n, cap, beginBit, endBit, st);
    if constexpr (HAS_V)
        return rocprim::radix_sort_pairs<RocCfg>(tmp, bytes, keysIn, keysOut, valsIn, valsOut, n, beginBit, endBit, st);
    else
        return rocprim::radix_sort_keys<RocCfg>(tmp, bytes, keysIn, keysOut, n, beginBit, endBit, st);
}

inline unsigned grid_for(size_t n, unsigned block = 256) { return (unsigned)((n + block - 1) / block); }
// bits that tell n values apart (the width of a radix sort's keys): at least one, at most `cap`
inline unsigned bits_for(uint64_t n, unsigned cap) {
    unsigned b = 1;
    while (b < cap && (1ull << b) < n)
        b++;
    return b;
}

// ---- the inspectors' segmented sum by key (deme_seg_sum.h): reserve, sort, sum ---------------------
// Room for n pairs: both halves, or only the half a select kernel writes (sorted false: nothing will sort them).
int seg_reserve(deme_ctx* c, SegPairs& p, size_t n, bool sorted = true) {
    for (int k = 0; k < (sorted ? 2 : 1); k++)
        if (ensure(c, p.key[k], n * 4) || ensure(c, p.val[k], n * 4))
            return c->lastStatus;
    return DEME_OK;
}
// The n pairs of half 0 into half 1, stably by keys 0 .. nKeys.
int seg_sort(deme_ctx* c, SegPairs& p, size_t n, size_t nKeys) {
    // (the key nKeys of the uncounted entries takes part: one value more than the keys)
    const unsigned bits = bits_for((uint64_t)nKeys + 1, 32);
    return with_temp(c, c->segTmp, [&](void* tmp, size_t& bytes) {
        return deme_radix_sort<DemeRadixCfg<8>, true>(tmp, bytes, p.key[0].as<uint32_t>(), p.key[1].as<uint32_t>(), p.val[0].as<uint32_t>(),
                                                      p.val[1].as<uint32_t>(), n, n, 0, bits, DEME_SORT_OWN_FROM_RECORDS, c->stream);
    });
}
// The sums of n sorted entries by key: term(e, v) reads what entry e adds (through the sorted values it holds), out.write stores a
// finished key.  The caller has cleared the outputs; nothing is launched for an empty list (a block reads the first entry of its
// range, so an empty list has no valid first block).
template <int L, class Term, class Out>
int seg_sums(deme_ctx* c, const uint32_t* keys, size_t n, size_t nKeys, const Term& term, const Out& out) {
    if (!n)
        return DEME_OK;
    const unsigned grid = grid_for(n, SEG_BLOCK_ROWS);
    if (ensure(c, c->segPartial, (size_t)grid * 2 * sizeof(SegPartial<L>)))
        return c->lastStatus;
    SegPartial<L>* partial = c->segPartial.as<SegPartial<L>>();
    hipLaunchKernelGGL((k_seg_sums<L, Term, Out>), dim3(grid), dim3(256), 0, c->stream, (uint32_t)n, (uint32_t)nKeys, keys, term, out, partial);
    hipLaunchKernelGGL((k_seg_final<L, Out>), dim3(1), dim3(256), 0, c->stream, 2u * grid, (uint32_t)nKeys, (const SegPartial<L>*)partial, out);
    return DEME_OK;
}
template <int L, class Term, class Out>
int seg_sums(deme_ctx* c, const SegPairs& p, size_t n, size_t nKeys, const Term& term, const Out& out) {
    return seg_sums<L>(c, p.key[1].as<uint32_t>(), n, nKeys, term, out);
}

// ---- kernel timing (HIP events on the context stream) ------------------------------------------
hipEvent_t get_event(deme_ctx* c) {
    if (!c->eventPool.empty()) {
        hipEvent_t e = c->eventPool.back();
        c->eventPool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
struct ScopedTimer {
    deme_ctx* c;
    TimerSlot* slot = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t st = nullptr;
    ScopedTimer(deme_ctx* ctx, const char* name, bool always = false, hipStream_t stream = nullptr) : c(ctx), st(stream ? stream : ctx->stream) {
        if (!c->timing)
            return;
        slot = &c->timers[name];
        if (!always && (slot->seen++ % (uint64_t)c->timing) != 0) {  // sampled: an event pair costs ~3 us of dispatch gap per launch
            slot = nullptr;
            return;
        }
        if (slot->pending.size() >= 8192) {  // bounded bookkeeping
            slot = nullptr;
            return;
        }
        a = get_event(c);
        b = get_event(c);
        hipEventRecord(a, st);
    }
    ~ScopedTimer() {
        if (slot) {
            hipEventRecord(b, st);
            slot->pending.emplace_back(a, b);
        }
    }
};
void drain_timers(deme_ctx* c) {
    for (auto& kv : c->timers) {
        for (auto& pr : kv.second.pending) {
            hipEventSynchronize(pr.second);
            float ms = 0;
            hipEventElapsedTime(&ms, pr.first, pr.second);
            kv.second.total_ms += ms;
            kv.second.launches++;
            c->eventPool.push_back(pr.first);
            c->eventPool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}

void refresh_dev_params(deme_ctx* c) {
    DevParams& d = c->dp;
    const DemeParams& h = c->hp;
    d.nvXp2 = h.nvXp2, d.nvYp2 = h.nvYp2;
    d.nbX = h.nbX, d.nbY = h.nbY, d.nbZ = h.nbZ;
    d.mNbX = fast_div_magic(h.nbX), d.mNbXY = fast_div_magic(h.nbX * h.nbY);
    d.l = h.l, d.voxelSize = h.voxelSize, d.binSize = h.binSize;
    d.LBFX = h.LBFX, d.LBFY = h.LBFY, d.LBFZ = h.LBFZ;
    d.Gx = h.Gx, d.Gy = h.Gy, d.Gz = h.Gz;
    d.h = h.h;
    d.approxMaxVel = h.approxMaxVel, d.expSafetyMulti = h.expSafetyMulti, d.expSafetyAdder = h.expSafetyAdder;
    d.errOutVel = h.errOutVel;
    d.integrator = h.integrator, d.forceModel = h.forceModel, d.nW = h.nContactWildcards;
    d.nOwners = c->nOwners, d.nSpheres = c->nSpheres, d.nAnal = c->nAnal, d.nMat = c->nMat;
    d.errOutBinSphNum = h.errOutBinSphNum ? h.errOutBinSphNum : 32768u;
    d.comp = c->comp.as<float4>();
    d.massProps = c->massProps.as<float4>();
    d.anal = c->anal.as<AnalObj>();
    d.matPair = c->matPair.as<MatPair>();
    d.E = c->E.as<float>(), d.nu = c->nu.as<float>(), d.CoR = c->CoR.as<float>(), d.mu = c->mu.as<float>(),
    d.Crr = c->Crr.as<float>();
    d.familyMasks = c->famMasks.as<uint8_t>();
    d.familyExtra = c->famExtra.as<float>();
    d.familyFlags = c->famFlags.as<uint8_t>();
    d.tris = c->tris.p;
    d.nTri = c->nTri;
    d.s2e = c->permuted ? c->dS2E.as<uint32_t>() : nullptr;
    d.o2e = c->permuted ? c->dO2E.as<uint32_t>() : nullptr;
}

int check_ready(deme_ctx* c) {
    if (!c)
        return DEME_ERR_INVALID;
    if (!c->haveParams || !c->haveScene)
        return fail(c, DEME_ERR_INVALID, "deme_set_params and deme_upload_scene must be called first");
    // (a process may hold contexts on several devices -- deme_multi: every entry point works on the context's own device)
    if (hipSetDevice(c->device) != hipSuccess)
        return fail(c, DEME_ERR_HIP, "device %d cannot be selected", c->device);
    return DEME_OK;
}

// per-material-pair constants of the Hertzian models, evaluated once on the host with the formulas
// of kernel/DEMHelperKernels.cuh:433-445 (matProxy2ContactParam<float>) and
// FullHertzianForceModel.cu:56-57 (loge, beta).  Host overload resolution (log/sqrt in double) as in
// the pinned reference build.
void build_mat_pairs(const DemeScene* s, std::vector<MatPair>& out) {
    const uint32_t n = s->nMat;
    out.resize((size_t)n * n);
    for (uint32_t a = 0; a < n; a++)
        for (uint32_t b = 0; b < n; b++) {
            MatPair m{};
            const float Y1 = s->E[a], nu1 = s->nu[a], Y2 = s->E[b], nu2 = s->nu[b];
            const float invE = (1.0f - nu1 * nu1) / Y1 + (1.0f - nu2 * nu2) / Y2;
            m.E_cnt = 1.0f / invE;
            const float invG = 2.0f * (2.0f - nu1) * (1.0f + nu1) / Y1 + 2.0f * (2.0f - nu2) * (1.0f + nu2) / Y2;
            m.G_cnt = 1.0f / invG;
            m.CoR = s->CoR ? s->CoR[a * n + b] : 0.f;
            m.mu = s->mu ? s->mu[a * n + b] : 0.f;
            m.Crr = s->Crr ? s->Crr[a * n + b] : 0.f;
            const float loge = (float)((m.CoR < 1e-12) ? log(1e-12) : logf(m.CoR));  // log(float) -> float overload
            m.beta = (float)(loge / sqrt(loge * loge + 9.869604401089358));
            out[(size_t)a * n + b] = m;
        }
}

// ---- the sizes of a contact list's buffers: ONE statement each for the per-contact and the per-owner / per-tile ones, used for
// the current list (grow_contact_arena, owner_scratch_for_counts) and for the one an asynchronous detection builds (async_size_next)
int size_list_per_contact(deme_ctx* c, ContactList& L, size_t cap, bool hasGhosts, uint32_t nTri) {
    int rc = 0;
    rc |= ensure(c, L.mapping, cap * 4, true);  // (read by the history migration after the detection that wrote it: kept)
    rc |= ensure(c, L.ownerA, cap * 4);
    for (int k = 0; k < 2; k++) {
        rc |= ensure(c, L.ownerB[k], cap * 4);
        rc |= ensure(c, L.bIdx[k], cap * 4);
    }
    rc |= ensure(c, L.info, cap * 16);
    rc |= ensure(c, L.tInfo, cap * 8);
    rc |= ensure(c, L.rIdx, cap * 4);
    rc |= ensure(c, L.lPos, cap * 2);
    rc |= ensure(c, L.remVal, (cap + 1) * 4);
    rc |= ensure(c, L.rankC, (cap + 1) * 4);
    rc |= ensure(c, L.remKey[0], (cap + 1) * 4);
    rc |= ensure(c, L.remKey[1], (cap + 1) * 4);
    if (hasGhosts) {
        rc |= ensure(c, L.cDefer, cap);
        rc |= ensure(c, L.blockMode, (cap / DEME_FORCE_BLOCK + 2) * 4);
    }
    if (nTri) {
        rc |= ensure(c, L.smFlag, cap);
        rc |= ensure(c, L.smList, cap * 4);
    }
    return rc;
}
int size_list_per_owner(deme_ctx* c, ContactList& L, size_t nO) {
    if (ensure(c, L.aStart, (nO + 1) * 4) || ensure(c, L.bStart, (nO + 1) * 4) || ensure(c, L.heavy, nO + 1) || ensure(c, L.fixedFlag, nO + 1) ||
        ensure(c, L.heavyList, 4096 * 4) || ensure(c, L.rangeCtr, sizeof(RangeCounters)))
        return c->lastStatus;
    const size_t nTiles = (nO + DEME_TILE_NB - 1) / DEME_TILE_NB + 1;
    if (ensure(c, L.hList, nTiles * DEME_TILE_HMAX * 4) || ensure(c, L.hCount, nTiles * 4) || ensure(c, L.tileMode, nTiles * 4) ||
        ensure(c, L.tileOrg, nTiles * 24) || ensure(c, L.rStart, (nO + 1) * 4) || ensure(c, L.lOff, nTiles * (DEME_TILE_NB + 1) * 2) ||
        ensure(c, L.lCount, nTiles * 4) || ensure(c, L.tileRem, (nTiles + 1) * 4) || ensure(c, L.tileBase, (nTiles + 1) * 4) ||
        ensure(c, L.tileBig, nTiles * 4) || ensure(c, L.bigList, nTiles * 4))
        return c->lastStatus;
    return DEME_OK;
}

int grow_contact_arena(deme_ctx* c, size_t cap) {
    const uint32_t nW = std::max<uint32_t>(c->hp.nContactWildcards, 1);
    int rc = 0;
    rc |= ensure(c, c->keysRaw, cap * 8);
    // sorted lists and wildcards carry state between detections: keep their contents
    rc |= ensure(c, c->keysSorted[0], cap * 8, true);
    rc |= ensure(c, c->keysSorted[1], cap * 8, true);
    rc |= ensure(c, c->wc[0], cap * 4 * nW, true);
    rc |= ensure(c, c->wc[1], cap * 4 * nW, true);
    if (c->record)
        for (int k = 0; k < 4; k++)
            rc |= ensure(c, c->rec[k], cap * 12);
    rc |= ensure(c, c->conA4, cap * 16);
    rc |= ensure(c, c->conA2, cap * 8);
    rc |= ensure(c, c->conB4, cap * 16);
    rc |= ensure(c, c->conB2, cap * 8);
    rc |= size_list_per_contact(c, c->list[c->cur], cap, c->hasGhosts, c->nTri);
    rc |= ensure(c, c->recContact, (cap + 1) * 4);
    rc |= ensure(c, c->tInfoIn, cap * 8);
    rc |= ensure(c, c->inContact, cap * 4);
    rc |= ensure(c, c->rec32, cap * 32);
    if (rc)
        return rc;
    c->cntCap = cap;
    return DEME_OK;
}

int grow_incidence_arena(deme_ctx* c, size_t cap) {
    int rc = 0;
    for (int k = 0; k < 2; k++) {
        rc |= ensure(c, c->incKeys[k], cap * 4);
        rc |= ensure(c, c->incVals[k], cap * 4);
    }
    if (rc)
        return rc;
    c->incCap = cap;
    return DEME_OK;
}

int status_to_error(deme_ctx* c, uint32_t st) {
    if (st & DEME_ST_NONFINITE)
        return fail(c, DEME_ERR_VELOCITY, "a non-finite owner velocity was found at time %.9g", c->timeElapsed);
    if (st & DEME_ST_VELOCITY)
        return fail(c, DEME_ERR_VELOCITY,
                    "system max velocity exceeded the error-out velocity %.7g at time %.9g (SetErrorOutVelocity)",
                    (double)c->hp.errOutVel, c->timeElapsed);
    return DEME_OK;
}

// The margins of the owner records `ow` for `drift` steps, on `st`.  The fill in front zeroes the detection's counters (the whole
// DetectBlock, the segment counters with it) and the kernel may leave status bits in them (velocity limit, non-finite state):
// the detection that follows does not zero them again, and the status comes back with its first read-back.
int launch_margins(deme_ctx* c, hipStream_t st, OwnerRec* ow, uint32_t drift) {
    HIPCK(hipMemsetAsync(c->ctr.p, 0, sizeof(DetectBlock), st));
    if (c->nOwners)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
        hipLaunchKernelGGL(k_margins, dim3(grid_for(c->nOwners)), dim3(256), 0, st, c->dp, ow, drift, c->ctr.as<DetectCounters>());
    c->ctrFresh = true;
    return DEME_OK;
}
int do_margins(deme_ctx* c, uint32_t drift) {
    return launch_margins(c, c->stream, c->owners.as<OwnerRec>(), drift);
}

int do_migrate(deme_ctx* c);

// What the stages of part 1 share: the caller's choices, the raw key arena of this attempt, the sizes read so far.
struct DetectRun {
    hipStream_t st;
    OwnerRec* ow;
    bool async;               // beside the steps, on the detection stream: the waits block instead of polling
    bool statusSeen = false;  // the status word the margins kernel left has been examined
    KeyArena ar{};
    bool segmented = false;
    uint32_t P = 0;              // (bin, sphere) incidences
    uint32_t nStats = 0, compactBlocks = 0;  // k_sweep's window records still to be added up; slot-blocks the early k_compact_keys covered
    uint64_t raw = 0, segMax = 0;            // keys the emitting kernels counted: in all, in the longest segment
    DetectCounters hc{};
};
inline unsigned bin_id_bits(const deme_ctx* c) { return bits_for((uint64_t)c->hp.nbX * c->hp.nbY * c->hp.nbZ, 32); }

// The raw key arena: 64 segments with a counter each once it is large enough for every segment to hold a fair share of any list
// (see KeyArena); one segment, counted in DetectCounters::nContactsRaw, below that.
void open_key_arena(deme_ctx* c, DetectRun& d) {
    DetectBlock* blk = c->ctr.as<DetectBlock>();
    d.segmented = c->keySegMin && c->cntCap >= c->keySegMin && c->cntCap >= DEME_KEY_SEGS * 64u;
    d.ar.keys = c->keysRaw.as<uint64_t>();
    d.ar.segMask = d.segmented ? DEME_KEY_SEGS - 1u : 0u;
    d.ar.segCap = d.segmented ? (uint64_t)c->cntCap / DEME_KEY_SEGS : (uint64_t)c->cntCap;
    d.ar.ctr = d.segmented ? blk->segCtr : &blk->c.nContactsRaw;
}

// Part 1's read-back: `bytes` of the counter block (sizeof(DetectHead): with the segments' counts), the counters also in d.hc.
// The first one of a detection brings the status the margins kernel left.  nullptr: failed, the code is in c->lastStatus.
const DetectHead* read_detect_counters(deme_ctx* c, DetectRun& d, size_t bytes) {
    const DetectHead* hh = read_back<DetectHead>(c, PIN_DETECT, c->ctr.p, d.st, !d.async, bytes);
    if (!hh || (!d.statusSeen && status_to_error(c, hh->c.status & ~DEME_ST_INCIDENCE)))
        return nullptr;
    d.statusSeen = true;
    d.hc = hh->c;
    return hh;
}

// Stage 1, the (bin, sphere) incidences: bounds and counts per sphere, their prefix, the pairs themselves.  Leaves d.P.
int detect_sphere_incidences(deme_ctx* c, DetectRun& d) {
    const uint32_t nS = c->nSpheres;
    d.P = 0;
    auto fill_incidence = [&]() {
        hipLaunchKernelGGL(k_fill_incidence, dim3(grid_for(nS)), dim3(256), 0, d.st, c->dp, c->binLo.as<uint4>(), c->binN.as<uint2>(),
                           c->binPartial.as<uint32_t>(), c->incKeys[0].as<uint32_t>(), c->incVals[0].as<uint32_t>(), (uint64_t)c->incCap);
    };
    if (nS) {
        c->geoStale = false;
        hipLaunchKernelGGL(k_sphere_prep, dim3(grid_for(nS)), dim3(256), 0, d.st, c->dp, d.ow, c->spheres.as<SphereRec>(),
                           c->geo.as<GeoRec>(), c->binLo.as<uint4>(), c->binN.as<uint2>(), c->binPartial.as<uint32_t>(), d.ar,
                           c->ctr.as<DetectCounters>(), c->sphFam.as<uint16_t>());
        // (one workgroup: the prefix of one sum per workgroup above, and the total for the read-back below)
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(DEME_SCAN_T), 0, d.st, c->binPartial.as<uint32_t>(), c->binPartial.as<uint32_t>(),
                           grid_for(nS), &c->ctr.as<DetectBlock>()->c.nIncidence);
        // the incidences go out before the host knows how many there are (the kernel guards the arena's end): the GPU works
        // through the read-back instead of idling
        const bool early = c->incCap != 0;
        if (early)
            fill_incidence();
        if (!read_detect_counters(c, d, sizeof(DetectCounters)))
            return c->lastStatus;
        if (d.hc.status & DEME_ST_INCIDENCE)
            return fail(c, DEME_ERR_OVERFLOW,
                        "a sphere touches more than %u bins (margin far larger than the bin size): the incidence list cannot be built",
                        DEME_MAX_BINS_PER_SPHERE);
        if (d.hc.nIncidence > 0xFFFFFFFFull)  // (the total is exact in 64 bits; the offsets the kernels work with have wrapped)
            return fail(c, DEME_ERR_OVERFLOW, "%llu bin-sphere incidences do not fit the 32-bit list offsets (use larger bins)",
                        d.hc.nIncidence);
        d.P = (uint32_t)d.hc.nIncidence;
        const bool grow = d.P > c->incCap;
        if (grow)
            if (int rc = grow_incidence_arena(c, (size_t)d.P + d.P / 4 + 1024))
                return rc;
        if (d.P && (grow || !early))  // (the early fill stopped at the old arena's end, or there was no arena to fill)
            fill_incidence();
    }
    c->nInc = d.P;
    return DEME_OK;
}

// Stage 2: the incidences sorted by bin, the sweep over each bin's spheres (it appends the sphere-sphere keys), and the windows'
// statistics (bins in use, the fullest bin) on their way to the counters.
int detect_sort_sweep(deme_ctx* c, DetectRun& d) {
    d.nStats = 0;
    if (!d.P)
        return DEME_OK;
    const uint32_t P = d.P;
    const hipStream_t st = d.st;
    const unsigned bits = bin_id_bits(c);
    // bin ids of up to 22 bits: two passes of 11 bits (16 keys per thread) take as long as three of 8 and save a pass's launches
    const bool twoPass = bits > 16 && bits <= 22;
    auto sort = [&](auto cfg, void* tmp, size_t& bytes) {
        return deme_radix_sort<decltype(cfg), true>(tmp, bytes, c->incKeys[0].as<uint32_t>(), c->incKeys[1].as<uint32_t>(), c->incVals[0].as<uint32_t>(),
                                                    c->incVals[1].as<uint32_t>(), (size_t)P, (size_t)c->incCap, 0, bits, DEME_SORT_OWN_FROM_INCIDENCES, st);
    };
    if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
            return twoPass ? sort(DemeRadixCfg<11, 16>{}, tmp, bytes) : sort(DemeRadixCfg<8>{}, tmp, bytes);
        }))
        return rc;
    const uint32_t nWin = (uint32_t)grid_for(P, SW_T);
    if (int rc = ensure(c, c->binStat, (size_t)nWin * sizeof(uint2)))
        return rc;
    static_assert(SW_WPB == 1, "k_sweep writes one statistics record per window");
    hipLaunchKernelGGL(k_sweep, dim3(nWin), dim3(SW_T), 0, st, c->dp, c->incKeys[1].as<uint32_t>(), c->incVals[1].as<uint32_t>(), P,
                       c->geo.as<GeoRec>(), c->sphFam.as<uint16_t>(), d.ar, c->binStat.as<uint2>());
    if (d.segmented)  // (the workgroups of k_compact_keys add the windows' statistics up)
        d.nStats = nWin;
    else
        hipLaunchKernelGGL(k_bin_stats_final, dim3((nWin + 2047u) / 2048u), dim3(256), 0, st, c->binStat.as<uint2>(), nWin,
                           c->ctr.as<DetectCounters>());
    return DEME_OK;
}

// Stage 3, sphere-triangle contacts (only when a mesh is loaded and some sphere is registered in a bin): the (bin, triangle)
// incidences, sorted by bin, swept against the spheres' (the sweep appends the sphere-mesh keys).
int detect_triangles(deme_ctx* c, DetectRun& d) {
    c->nTriInc = 0;
    if (!c->nTri || !d.P)
        return DEME_OK;
    const uint32_t nT = c->nTri;
    const hipStream_t st = d.st;
    hipLaunchKernelGGL(k_tri_prep, dim3(grid_for(nT)), dim3(256), 0, st, c->dp, nT, c->tris.as<TriRec>(), d.ow,
                       c->triWorld.as<TriWorld>(), c->triLo.as<int4>(), c->triHi.as<int4>(), c->triCounts.as<uint32_t>());
    if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->triCounts.as<uint32_t>(), c->triOffsets.as<uint32_t>(), 0u, (size_t)nT + 1,
                                           rocprim::plus<uint32_t>(), st);
        }))
        return rc;
    const uint32_t* tp = read_back<uint32_t>(c, PIN_TRI, c->triOffsets.as<uint32_t>() + nT, st, false);
    if (!tp)
        return c->lastStatus;
    const uint32_t TP = *tp;
    if (TP > c->triCap) {
        const size_t cap = (size_t)TP + TP / 4 + 1024;
        for (int k = 0; k < 2; k++)
            if (ensure(c, c->triKeys[k], cap * 4) || ensure(c, c->triVals[k], cap * 4))
                return c->lastStatus;
        c->triCap = cap;
    }
    c->nTriInc = TP;
    if (!TP)
        return DEME_OK;
    hipLaunchKernelGGL(k_tri_fill, dim3(grid_for(nT)), dim3(256), 0, st, c->dp, nT, c->triWorld.as<TriWorld>(), c->triLo.as<int4>(),
                       c->triHi.as<int4>(), c->triOffsets.as<uint32_t>(), c->triKeys[0].as<uint32_t>(), c->triVals[0].as<uint32_t>(),
                       (uint64_t)c->triCap);
    if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_pairs(tmp, bytes, c->triKeys[0].as<uint32_t>(), c->triKeys[1].as<uint32_t>(),
                                             c->triVals[0].as<uint32_t>(), c->triVals[1].as<uint32_t>(), (size_t)TP, 0, bin_id_bits(c), st);
        }))
        return rc;
    hipLaunchKernelGGL(k_tri_sweep, dim3(grid_for(TP)), dim3(256), 0, st, c->dp, TP, c->triKeys[1].as<uint32_t>(),
                       c->triVals[1].as<uint32_t>(), c->triWorld.as<TriWorld>(), d.P, c->incKeys[1].as<uint32_t>(),
                       c->incVals[1].as<uint32_t>(), c->geo.as<GeoRec>(), c->sphFam.as<uint16_t>(), d.ar);
    return DEME_OK;
}
// Stage 4, closing the arena: how many keys the emitting kernels counted (d.raw; d.segMax in the longest segment).  The gaps
// between the segments are closed while the host waits for the counts: a launch sized from the last detection's longest segment,
// the rest (if a segment grew past that) once the counts are known (detect_order_keys).
int detect_close_arena(deme_ctx* c, DetectRun& d) {
    d.compactBlocks = 0;
    if (d.segmented) {
        d.compactBlocks = (uint32_t)std::min<uint64_t>(grid_for(std::max<uint64_t>(c->lastSegMax + c->lastSegMax / 8 + 1024, 1)), grid_for(d.ar.segCap));
        hipLaunchKernelGGL(k_compact_keys, dim3(d.compactBlocks, DEME_KEY_SEGS), dim3(256), 0, d.st, c->keysRaw.as<uint64_t>(), d.ar.segCap,
                           c->ctr.as<DetectBlock>(), 0u, c->keysSorted[c->keysCur ^ 1].as<uint64_t>(), c->binStat.as<uint2>(), d.nStats);
    }
    // one copy: the counters and, with the segmented arena, the 64 counts k_compact_keys has put beside them
    const DetectHead* hh = read_detect_counters(c, d, d.segmented ? sizeof(DetectHead) : sizeof(DetectCounters));
    if (!hh)
        return c->lastStatus;
    d.raw = d.hc.nContactsRaw, d.segMax = 0;
    if (d.segmented) {
        d.raw = 0;
        for (uint32_t g = 0; g < DEME_KEY_SEGS; g++) {
            d.raw += hh->segCount[g];
            d.segMax = std::max<uint64_t>(d.segMax, hh->segCount[g]);
        }
    }
    return DEME_OK;
}

// The one rule by which the contact arena grows: the capacity that `raw` keys with `segMax` of them in one segment, and `marks`
// persistent keys appended behind them, ask of an arena of `cap` slots in segments of `segCap` -- or 0 when everything fits.
size_t contact_arena_wanted(uint64_t raw, uint64_t segMax, uint64_t segCap, size_t marks, size_t cap) {
    size_t grow = 0;
    if (raw > cap || segMax > segCap) {  // the arena, or one segment of it, is too small for the emitting kernels
        const size_t want = std::max<size_t>(raw, (size_t)segMax * DEME_KEY_SEGS);
        grow = want + want / 4 + 1024;
    }
    if (marks && raw + marks > std::max(cap, grow))  // ... or for the marked contacts behind what they emitted
        grow = (size_t)raw + marks + raw / 4 + 1024;
    return grow;
}

// Stage 5, ordering the keys: the rest of the compaction, the marked contacts (they join the list whether or not the sweep found
// them: DEMCubContactDetection.cu:605-802), and the list order in the next key buffer.  Returns the list's length in *nCout.
int detect_order_keys(deme_ctx* c, DetectRun& d, uint64_t* nCout) {
    const hipStream_t st = d.st;
    const size_t nPersist = c->hPersist.size();
    uint64_t nC = d.raw + nPersist;
    const int next = c->keysCur ^ 1;
    uint64_t* rawKeys = c->keysRaw.as<uint64_t>();
    if (d.segmented) {  // (the next list's buffer is free until the rank sort fills it)
        c->lastSegMax = d.segMax;
        if (grid_for(d.segMax) > d.compactBlocks)
            hipLaunchKernelGGL(k_compact_keys, dim3((unsigned)grid_for(d.segMax) - d.compactBlocks, DEME_KEY_SEGS), dim3(256), 0, st,
                               c->keysRaw.as<uint64_t>(), d.ar.segCap, c->ctr.as<DetectBlock>(), d.compactBlocks,
                               c->keysSorted[next].as<uint64_t>(), (const uint2*)nullptr, 0u);
        if (d.raw)
            rawKeys = c->keysSorted[next].as<uint64_t>();
    }
    if (nPersist)
        HIPCK(hipMemcpyAsync(rawKeys + d.raw, c->persistKeys.p, nPersist * 8, hipMemcpyDeviceToDevice, st));
    if (nC) {
        // key = A << 33 | class << 31 | B.  One radix sort over the occupied upper bits [31, 33 + bits(A)) groups the keys by
        // (sphere A, class) -- 3 passes at 3e6 spheres, where a full 64-bit order took 6 to 8 -- and k_segment_rank_sort puts each
        // group's few partners in order (DEMCubContactDetection.cu:811-1110 runs five full sorts for the same list order)
        const unsigned bitsA = bits_for(c->dp.nSpheres, 31);
        if (int rc = ensure(c, c->keysMid, (size_t)c->cntCap * 8))  // (its own scratch: an asynchronous detection runs beside force passes)
            return rc;
        uint64_t* mid = c->keysMid.as<uint64_t>();
        if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
                return deme_radix_sort<DemeRadixCfg<8>, false>(tmp, bytes, rawKeys, mid, nullptr, nullptr, (size_t)nC, (size_t)c->cntCap, 31,
                                                               33 + bitsA, DEME_SORT_OWN_FROM_KEYS64, st);
            }))
            return rc;
        hipLaunchKernelGGL(k_segment_rank_sort, dim3(grid_for(nC)), dim3(256), 0, st, (uint32_t)nC, mid,
                           c->keysSorted[next].as<uint64_t>());
        if (nPersist) {  // a marked contact the sweep found as well appears once (markDuplicateContacts)
            unsigned long long* cnt = &c->ctr.as<DetectBlock>()->c.nContactsRaw;
            if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
                    return rocprim::unique(tmp, bytes, c->keysSorted[next].as<uint64_t>(), c->keysRaw.as<uint64_t>(), cnt, (size_t)nC,
                                           rocprim::equal_to<uint64_t>(), st);
                }))
                return rc;
            const unsigned long long* nU = read_back<unsigned long long>(c, PIN_UNIQUE, cnt, st, false);
            if (!nU)
                return c->lastStatus;
            nC = *nU;
            HIPCK(hipMemcpyAsync(c->keysSorted[next].p, c->keysRaw.p, (size_t)nC * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    *nCout = nC;
    return DEME_OK;
}

// contactDetection() equivalent, in two parts.  Part 1 -- everything up to the sorted key list of the new contacts -- reads the
// owners through `ow` and touches detection scratch only, so it can run on its own stream from a snapshot of the owner records
// while the main stream keeps stepping with the current list (deme_set_async_detection; the reference's kT does the same on its
// own GPU thread).  Part 2 -- history map and the per-owner gather lists the force and integration kernels read -- runs on the
// main stream when the list is swapped in.
// Part 1 is an attempt repeated with a larger contact arena until every key has a slot: the stages above, and one decision.
int detect_part1(deme_ctx* c, hipStream_t st, OwnerRec* ow, bool async, uint64_t* nCout) {
    DetectRun d{st, ow, async};
    const bool countersFresh = c->ctrFresh;  // (launch_margins has just zeroed them and left its status there)
    c->ctrFresh = false;
    for (int attempt = 0; attempt < 4; attempt++) {
        if (attempt > 0 || !countersFresh)
            HIPCK(hipMemsetAsync(c->ctr.p, 0, sizeof(DetectBlock), st));
        open_key_arena(c, d);
        if (int rc = detect_sphere_incidences(c, d))
            return rc;
        if (int rc = detect_sort_sweep(c, d))
            return rc;
        if (int rc = detect_triangles(c, d))
            return rc;
        if (int rc = detect_close_arena(c, d))
            return rc;
        if (const size_t cap = contact_arena_wanted(d.raw, d.segMax, d.ar.segCap, c->hPersist.size(), c->cntCap)) {
            if (async)  // (the steps in flight read buffers of the arena)
                HIPCK(hipStreamSynchronize(c->stream));
            if (int rc = grow_contact_arena(c, cap))
                return rc;
            continue;  // the emitting kernels run again
        }
        c->nActiveBins = d.hc.nActiveBins;
        c->maxInBin = d.hc.maxInBin ? d.hc.maxInBin : (d.P ? 1u : 0u);
        if (c->maxInBin > c->dp.errOutBinSphNum)
            return fail(c, DEME_ERR_BIN_TOO_FULL,
                        "a bin contains %u sphere components, exceeding the allowance %u (SetMaxSphereInBin)", c->maxInBin,
                        c->dp.errOutBinSphNum);
        return detect_order_keys(c, d, nCout);
    }
    return fail(c, DEME_ERR_OVERFLOW, "contact arena kept overflowing");
}

// The B-sorted contact list of the round-2 kernels (k_forces_fast / k_calc_forces + the integrator's gather): owner-B sort, run
// starts, heavy / fixed flags, the deferral flags of the halo overlap.  Enqueued on `st`; the caller reads rangeCtr.
int build_legacy_lists(deme_ctx* c, ContactList& L, const OwnerRec* ow, hipStream_t st) {
    const uint64_t nC = L.nListed;
    if (nC) {
        const unsigned obits = bits_for(c->nOwners, 32);
        if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
                return rocprim::radix_sort_pairs(tmp, bytes, L.ownerB[0].as<uint32_t>(), L.ownerB[1].as<uint32_t>(), L.bIdx[0].as<uint32_t>(),
                                                 L.bIdx[1].as<uint32_t>(), (size_t)nC, 0, obits, st);
            }))
            return rc;
    }
    if (c->hasGhosts) {  // (the arena may have been sized before the scene's family flags were known)
        if (int rc = size_list_per_contact(c, L, c->cntCap, true, c->nTri))
            return rc;
        HIPCK(hipMemsetAsync(L.blockMode.p, 0, L.blockMode.bytes, st));
    }
    if (nC)
        hipLaunchKernelGGL(k_run_starts, dim3(grid_for(nC)), dim3(256), 0, st, (uint32_t)nC, L.ownerB[1].as<uint32_t>(),
                           c->nOwners, L.bStart.as<uint32_t>());
    else
        HIPCK(hipMemsetAsync(L.bStart.p, 0, ((size_t)c->nOwners + 1) * 4, st));
    // (the counters may hold the tile builders' count of the same owners)
    HIPCK(hipMemsetAsync(&L.rangeCtr.as<RangeCounters>()->nHeavy, 0, 2 * sizeof(unsigned int), st));
    hipLaunchKernelGGL(k_owner_ranges, dim3(grid_for((size_t)c->nOwners + 1)), dim3(256), 0, st, c->dp, (uint32_t)nC,
                       L.ownerA.as<uint32_t>(), L.ownerB[1].as<uint32_t>(), ow, L.aStart.as<uint32_t>(),
                       L.bStart.as<uint32_t>(), L.heavy.as<uint8_t>(), L.fixedFlag.as<uint8_t>(), L.heavyList.as<uint32_t>(),
                       (uint32_t)(L.heavyList.bytes / 4), L.rangeCtr.as<RangeCounters>(), L.info.as<uint4>(),
                       c->hasGhosts ? L.cDefer.as<uint8_t>() : (uint8_t*)nullptr, L.blockMode.as<uint32_t>());
    L.legacyLists = true;
    return DEME_OK;
}
// ... and its heavy-owner counts on the host (a wait for `st`)
int read_legacy_counts(deme_ctx* c, ContactList& L, hipStream_t st, RangeCounters& hr) {
    const RangeCounters* got = read_back<RangeCounters>(c, PIN_LEGACY, L.rangeCtr.p, st, false);
    if (!got)
        return c->lastStatus;
    hr = *got;
    if (hr.nHeavy > L.heavyList.bytes / 4)
        return fail(c, DEME_ERR_OVERFLOW, "%u owners exceed the heavy-owner list", hr.nHeavy);
    L.nHeavy = hr.nHeavy, L.nHeavyFree = hr.nHeavyFree;
    return DEME_OK;
}

void resolve_heavy_counts(deme_ctx* c, ContactList& L);
// a list built with tile structures that the round-2 kernels evaluate after all (contact recording switched on, the arithmetic
// mode changed ...): its B-sorted form is built now
int ensure_legacy_lists(deme_ctx* c) {
    ContactList& L = c->list[c->cur];
    if (L.legacyLists || !c->haveList)
        return DEME_OK;
    resolve_heavy_counts(c, L);
    if (int rc = build_legacy_lists(c, L, c->owners.as<OwnerRec>(), c->stream))
        return rc;
    RangeCounters hr{};
    return read_legacy_counts(c, L, c->stream, hr);
}

// May a list of nC contacts get tile structures (deme_tile.h)?  The fast mode; a user model only with its tile kernels compiled and
// enough contacts per tile to pay for them; no replicated free owners; tables that the tile kernels can stage.
inline uint32_t tile_count(const deme_ctx* c) { return (c->nOwners + DEME_TILE_NB - 1) / DEME_TILE_NB; }
bool tile_eligible(const deme_ctx* c, uint64_t nC) {
    const uint32_t nTiles = tile_count(c);
    if (!nC || c->arith != DEME_ARITH_FAST || !c->hShared.empty())
        return false;
    if (c->hp.forceModel == DEME_FORCE_CUSTOM && !(c->customTileFn[0] && nC >= (uint64_t)c->tileMinContactsCustom * nTiles))
        return false;
    // the tables are loaded in one round of 16-byte pieces, one per thread.  tInfo names a material in 4 bits: a table of 17 or
    // more materials has more pieces than a round by itself, so no test of nMat <= 16 is needed beside this one.
    static_assert(DEME_TILE_T < 2 * 17 * 17, "a tile's tables may hold more than 16 materials: tInfo has 4-bit material fields");
    const uint64_t pieces = (uint64_t)c->nComp + 2ull * c->nMat * c->nMat + 4ull * c->nAnal;
    return pieces <= DEME_TILE_T && c->nMassProps <= DEME_TILE_T && c->nAnal <= 65535 && c->nComp <= 65535 &&
           tile_table_bytes(c->nComp, c->nMat, c->nAnal, c->nMassProps, c->dp.familyTrivial) <= DEME_TILE_TABLE_MAX;
}
// May a tiled list whose counters read `hr` get the closed-tile structures of the one-kernel step (deme_tile_step.h)?  Switched on
// (DEME_FUSED = 1 / 0 overrides the context's switch for the whole process), every tile fits, the built-in models, and nothing
// the one kernel does not do: records, a mesh, ghosts, prescriptions, family rules, replicated owners, the adaptive controllers.
// Never with asynchronous detection on: the closed-tile structures exist once -- see deme_ctx.
bool fused_eligible(const deme_ctx* c, const RangeCounters& hr) {
    static const int fusedEnv = getenv("DEME_FUSED") ? atoi(getenv("DEME_FUSED")) : -1;
    const int fusedMode = fusedEnv < 0 ? c->fusedEnable : fusedEnv;  // 0 off, 1 on, 2 by the size of the bed
    return (fusedMode == 2 ? c->nOwners <= DEME_FUSED_AUTO_MAX_OWNERS : fusedMode != 0) && hr.nBig == 0 &&
           c->hp.forceModel != DEME_FORCE_CUSTOM && !c->record && c->nTri == 0 && !c->hasGhosts && !c->prescFn && !c->rulesFn &&
           c->hShared.empty() && c->asyncLead == 0 && !c->ad.autoBinSize && !c->ad.autoUpdateFreq;
}

// ---- part 2 of a detection, piece by piece: each builds structures of `L` on `st` and touches nothing else of the context
// The history map of the nC keys in the next key buffer against the current list, the owners of every contact, the work list of
// the mesh-variant force kernel and the starts of the A owners' runs.
int build_owner_arrays(deme_ctx* c, ContactList& L, hipStream_t st, uint64_t nC, bool tileEligible) {
    const int next = c->keysCur ^ 1;
    const uint32_t nTiles = tile_count(c);
    if (nC) {
        const uint64_t nPrev = c->haveList ? c->nContacts : 0;
        hipLaunchKernelGGL(k_history, dim3(grid_for(nC)), dim3(256), 0, st, (uint32_t)nC, c->keysSorted[next].as<uint64_t>(),
                           (uint32_t)nPrev, c->keysSorted[c->keysCur].as<uint64_t>(), L.mapping.as<uint32_t>(),
                           L.rangeCtr.as<uint32_t>(), (uint32_t)(sizeof(RangeCounters) / 4), L.tileRem.as<uint32_t>(),
                           tileEligible ? nTiles + 1 : 0u);
    } else {  // (k_history zeroes the list builders' counters on the side; no list, no tiles)
        HIPCK(hipMemsetAsync(L.rangeCtr.p, 0, sizeof(RangeCounters), st));
    }
    // per-owner gather lists for the atomics-free accumulation
    if (nC) {
        hipLaunchKernelGGL(k_contact_owners, dim3(grid_for(nC)), dim3(256), 0, st, c->dp, (uint32_t)nC,
                           c->keysSorted[next].as<uint64_t>(), c->spheres.as<SphereRec>(), L.ownerA.as<uint32_t>(),
                           L.ownerB[0].as<uint32_t>(), L.bIdx[0].as<uint32_t>(), L.info.as<uint4>(),
                           c->nTri ? L.smFlag.as<uint8_t>() : (uint8_t*)nullptr,
                           tileEligible ? L.tileRem.as<uint32_t>() : (uint32_t*)nullptr, (uint32_t)DEME_TILE_NB);
        if (c->nTri) {  // work list of the mesh-variant force kernel; its length lands in RangeCounters::nSM
            unsigned int* cnt = &L.rangeCtr.as<RangeCounters>()->nSM;
            if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
                    return rocprim::select(tmp, bytes, rocprim::counting_iterator<uint32_t>(0), L.smFlag.as<uint8_t>(), L.smList.as<uint32_t>(), cnt,
                                           (size_t)nC, st);
                }))
                return rc;
        }
        hipLaunchKernelGGL(k_run_starts, dim3(grid_for(nC)), dim3(256), 0, st, (uint32_t)nC, L.ownerA.as<uint32_t>(), c->nOwners,
                           L.aStart.as<uint32_t>());
    } else {
        HIPCK(hipMemsetAsync(L.aStart.p, 0, ((size_t)c->nOwners + 1) * 4, st));
    }
    L.nListed = nC, L.listKeys = next;
    return DEME_OK;
}
// Owner tiles (deme_tile.h): the list structures k_tile_forces and the integrator read.  `hr`: the counters as the host needs them
// in the middle -- the tiles' extremes and the number of crossing contacts, the one size the sort of their records has to know.
int build_tiles(deme_ctx* c, ContactList& L, const OwnerRec* ow, hipStream_t st, RangeCounters& hr) {
    const uint32_t nTiles = tile_count(c);
    hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(DEME_SCAN_T), 0, st, L.tileRem.as<uint32_t>(), L.tileBase.as<uint32_t>(), nTiles + 1,
                       &L.rangeCtr.as<RangeCounters>()->nRemote);
    hipLaunchKernelGGL(k_tile_build, dim3(nTiles), dim3(256), 0, st, c->dp, c->nOwners, L.info.as<uint4>(),
                       L.ownerB[0].as<uint32_t>(), L.aStart.as<uint32_t>(), ow, L.tileBase.as<uint32_t>(), L.tInfo.as<uint2>(),
                       L.hList.as<uint32_t>(), L.hCount.as<uint32_t>(),
                       c->hasGhosts ? L.tileMode.as<uint32_t>() : (uint32_t*)nullptr, L.lOff.as<uint16_t>(),
                       L.lPos.as<uint16_t>(), L.lCount.as<uint32_t>(), L.rankC.as<uint32_t>(), L.remKey[0].as<uint32_t>(),
                       L.remVal.as<uint32_t>(), L.tileOrg.as<int64_t>(), L.rangeCtr.as<RangeCounters>(), nTiles,
                       L.tileBig.as<uint32_t>(), L.bigList.as<uint32_t>(), c->recContact.as<uint32_t>());
    hipLaunchKernelGGL(k_tile_stats, dim3((nTiles + 1023u) / 1024u), dim3(256), 0, st, nTiles, L.hCount.as<uint32_t>(),
                       L.lCount.as<uint32_t>(), L.rangeCtr.as<RangeCounters>());
    const RangeCounters* got = read_back<RangeCounters>(c, PIN_RANGES, L.rangeCtr.p, st, true);  // (part 2 is short, also beside the steps)
    if (!got)
        return c->lastStatus;
    hr = *got;
    // crossing contacts = records = entries of the sort below
    // (nExtra: the records of the tiles that do not fit (k_tile_forces_big): every contact of such a tile has one)
    const uint32_t nR = (uint32_t)hr.nRemote + hr.nExtra;
    L.nBigTiles = hr.nBig;
    const unsigned obits = bits_for(c->nOwners, 32);
    if (nR) {
        if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
                return deme_radix_sort<DemeRadixCfg<10>, true>(tmp, bytes, L.remKey[0].as<uint32_t>(), L.remKey[1].as<uint32_t>(),
                                                               L.remVal.as<uint32_t>(), L.rIdx.as<uint32_t>(), (size_t)nR, (size_t)c->cntCap, 0, obits,
                                                               DEME_SORT_OWN_FROM_RECORDS, st);
            }))
            return rc;
        hipLaunchKernelGGL(k_run_starts, dim3(grid_for(nR)), dim3(256), 0, st, nR, L.remKey[1].as<uint32_t>(), c->nOwners,
                           L.rStart.as<uint32_t>());
    } else {
        HIPCK(hipMemsetAsync(L.rStart.p, 0, ((size_t)c->nOwners + 1) * 4, st));
    }
    hipLaunchKernelGGL(k_owner_ranges_tile, dim3(grid_for(c->nOwners)), dim3(256), 0, st, c->dp, ow, L.aStart.as<uint32_t>(),
                       L.lOff.as<uint16_t>(), L.rStart.as<uint32_t>(), L.heavy.as<uint8_t>(), L.fixedFlag.as<uint8_t>(),
                       L.heavyList.as<uint32_t>(), (uint32_t)(L.heavyList.bytes / 4), L.rangeCtr.as<RangeCounters>());
    return DEME_OK;
}
// Closed tiles (deme_tile_step.h): the contacts that hold a tile's owners as B from other tiles, in the tile's frame.  Whether
// every closed tile fits comes back with the pending heavy-owner counts (resolve_heavy_counts).
int build_closed_tiles(deme_ctx* c, ContactList& L, const OwnerRec* ow, hipStream_t st) {
    const uint32_t nTiles = tile_count(c);
    hipLaunchKernelGGL(k_in_count, dim3(grid_for((size_t)c->nOwners + 1)), dim3(256), 0, st, c->dp, ow,
                       L.rStart.as<uint32_t>(), c->inCnt.as<uint32_t>());
    if (int rc = with_temp(c, c->scanTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::exclusive_scan(tmp, bytes, c->inCnt.as<uint32_t>(), c->inStart.as<uint32_t>(), 0u, (size_t)c->nOwners + 1,
                                           rocprim::plus<uint32_t>(), st);
        }))
        return rc;
    hipLaunchKernelGGL(k_tile_incoming, dim3(nTiles), dim3(256), 0, st, c->dp, c->nOwners, L.info.as<uint4>(),
                       L.rStart.as<uint32_t>(), L.rIdx.as<uint32_t>(), c->recContact.as<uint32_t>(), c->inStart.as<uint32_t>(),
                       L.hList.as<uint32_t>(), L.hCount.as<uint32_t>(), c->hCountIn.as<uint32_t>(), c->tInfoIn.as<uint2>(),
                       c->inContact.as<uint32_t>(), L.rangeCtr.as<RangeCounters>());
    L.fusedList = true;
    return DEME_OK;
}
// The heavy-owner counts of a tiled list are fetched without stopping the stream: the first reader waits for the event
// (resolve_heavy_counts, one force launch later).
int fetch_heavy_counts(deme_ctx* c, ContactList& L, hipStream_t st) {
    if (!c->hrEvent)
        HIPCK(hipEventCreateWithFlags(&c->hrEvent, hipEventDisableTiming));
    HIPCK(hipMemcpyAsync(pin_at<RangeCounters>(c, PIN_HEAVY), L.rangeCtr.p, sizeof(RangeCounters), hipMemcpyDeviceToHost, st));
    HIPCK(hipEventRecord(c->hrEvent, st));
    L.hrPending = true;
    return DEME_OK;
}
// The list of nC contacts is built (in list[cur], or in the list the caller is about to flip to): the context turns to it.
void commit_list(deme_ctx* c, uint64_t nC) {
    c->fusedPrevValid = false;  // (a replay of the last fused step would read the list it was taken with)
    c->conValid = false;
    c->nPrev = c->haveList ? c->nContacts : 0;
    c->nContacts = nC;
    c->keysCur ^= 1;
    c->listSerial++;
    c->haveList = true;
    c->seeded = false;
    c->mapFresh = true;
    c->nDetections++;
}

void order_watch_drift(deme_ctx* c, const RangeCounters& hr);  // (deme_order.inc)
// Part 2 of a detection: the history map and the structures of `L`, built on `st` from the owner records `ow` (the live ones --
// or, beside steps that are integrating them, the snapshot part 1 was made from) and the nC keys part 1 left in the next key
// buffer.  Everything fallible comes first and touches `L` only; the two calls at the end cannot fail and turn the context.
int detect_part2(deme_ctx* c, ContactList& L, const OwnerRec* ow, hipStream_t st, uint64_t nC) {
    L.invalidate();  // (a pending read-back of this list's last build is superseded)
    const bool tiled = tile_eligible(c, nC);
    RangeCounters hr{};
    if (int rc = build_owner_arrays(c, L, st, nC, tiled))
        return rc;
    if (tiled) {
        if (int rc = build_tiles(c, L, ow, st, hr))
            return rc;
        if (fused_eligible(c, hr))
            if (int rc = build_closed_tiles(c, L, ow, st))
                return rc;
        if (int rc = fetch_heavy_counts(c, L, st))  // (hr holds the tile extremes already; nSA / nSM are not used by the tile path)
            return rc;
    } else {
        if (int rc = build_legacy_lists(c, L, ow, st))
            return rc;
        if (int rc = read_legacy_counts(c, L, st, hr))
            return rc;
    }
    L.tileActive = tiled;
    L.tileMaxHalo = hr.tileMaxHalo, L.tileMaxList = hr.tileMaxList;
    L.nSA = hr.nSA;
    L.nSM = hr.nSM;
    if (tiled)
        order_watch_drift(c, hr);
    commit_list(c, nC);
    return DEME_OK;
}


int do_detect(deme_ctx* c) {
    // a history map nobody has applied yet (two detections in a row): apply it now, or the next map would be taken from a
    // list whose wildcards are still stored against the list before it
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    ScopedTimer tm(c, "detect", true);  // once per K steps: always timed
    uint64_t nC = 0;
    if (int rc = detect_part1(c, c->stream, c->owners.as<OwnerRec>(), false, &nC))
        return rc;
    return detect_part2(c, c->list[c->cur], c->owners.as<OwnerRec>(), c->stream, nC);
}

int do_migrate(deme_ctx* c) {
    ContactList& L = c->list[c->cur];
    const uint32_t nW = c->hp.nContactWildcards;
    if (!c->mapFresh)
        return DEME_OK;
    c->mapFresh = false;
    if (nW == 0) {
        c->nWcStored = c->nContacts;
        return DEME_OK;
    }
    const int next = c->wcCur ^ 1;
    if (c->nContacts)
        hipLaunchKernelGGL(k_migrate, dim3(grid_for(c->nContacts)), dim3(256), 0, c->stream, (uint32_t)c->nContacts, nW,
                           L.mapping.as<uint32_t>(), (uint32_t)c->nWcStored, c->wc[c->wcCur].as<float>(),
                           c->wc[next].as<float>());
    c->wcCur = next;
    c->nWcStored = c->nContacts;
    return DEME_OK;
}

GatherArgs gather_args(deme_ctx* c) {
    ContactList& L = c->list[c->cur];
    GatherArgs g{};
    g.aStart = L.aStart.as<uint32_t>(), g.bStart = L.bStart.as<uint32_t>(), g.bIdx = L.bIdx[1].as<uint32_t>();
    g.heavy = L.heavy.as<uint8_t>();
    g.conA4 = c->conA4.as<float4>(), g.conA2 = c->conA2.as<float2>();
    g.conB4 = c->conB4.as<float4>(), g.conB2 = c->conB2.as<float2>();
    g.aSum = c->aSum.as<float4>();
    g.nextAcc = c->nextAccPending ? c->nextAcc.as<AccRec>() : nullptr;
    if (c->pairsOnce && c->revAcc)
        g.revSlot = c->revSlot.as<uint32_t>(), g.revAcc = (const float4*)c->revAcc;
    g.world = c->arith == DEME_ARITH_FAST ? 1u : 0u;
    if (c->conTile) {  // the tile kernel's sums and its records of tile-crossing contacts
        g.bStart = L.rStart.as<uint32_t>(), g.bIdx = L.rIdx.as<uint32_t>();
        g.rec32 = c->rec32.as<float4>();
        g.tile = 1u;
    }
    return g;
}

// heavy owners: skipFixed=true in the stepping loop (a fixed owner's a/alpha are only needed by queries)
void resolve_heavy_counts(deme_ctx* c, ContactList& L) {
    if (!L.hrPending)
        return;
    L.hrPending = false;
    if (const hipError_t e = hipEventSynchronize(c->hrEvent); e != hipSuccess) {
        fail(c, DEME_ERR_HIP, "waiting for the heavy-owner counts: %s", hipGetErrorString(e));
        L.heavyOverflow = true;  // (the stepping loop returns the error: launch_integrate)
        return;
    }
    const size_t cap = L.heavyList.bytes / 4;
    const RangeCounters* hr = pin_at<RangeCounters>(c, PIN_HEAVY);
    L.nHeavy = hr->nHeavy, L.nHeavyFree = hr->nHeavyFree;
    if (L.fusedList) {  // the halos were extended by the incoming contacts' owners (k_tile_incoming): the kernels' LDS follows
        L.tileMaxHaloIn = hr->tileMaxHaloIn;
        if (hr->nBigIn)  // a closed tile does not fit: this list keeps force pass + integrator
            L.fusedList = false;
        L.fusedChecked = true;
    }
    if (L.nHeavy > cap) {
        fail(c, DEME_ERR_OVERFLOW, "%u owners exceed the heavy-owner list", L.nHeavy);
        L.nHeavy = (uint32_t)cap;
        L.heavyOverflow = true;  // (the stepping loop returns the error)
    }
}

void launch_reduce_heavy(deme_ctx* c, bool skipFixed) {
    ContactList& L = c->list[c->cur];
    resolve_heavy_counts(c, L);
    if (L.nHeavy == 0 || (skipFixed && L.nHeavyFree == 0))
        return;
    hipLaunchKernelGGL(k_reduce_heavy, dim3(std::min<uint32_t>(L.nHeavy, 1024)), dim3(256), 0, c->stream, c->dp, gather_args(c),
                       c->owners.as<OwnerRec>(), L.heavyList.as<uint32_t>(), &L.rangeCtr.as<RangeCounters>()->nHeavy,
                       skipFixed ? L.fixedFlag.as<uint8_t>() : (const uint8_t*)nullptr, c->acc.as<AccRec>());
}

// the XCD-aware block maps of the force kernels are bijections on multiples of 8 G blocks (G = DevParams' xcdGroup; 0: no map)
inline unsigned xcd_round(unsigned nBlk, uint32_t G) { return G ? (nBlk + 8u * G - 1u) / (8u * G) * (8u * G) : nBlk; }

// a run-time bool as a type: f(std::true_type) or f(std::false_type), for picking a kernel instance
template <class F>
void as_constant(bool b, F&& f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// the model class of a launch: 0 / 1 the built-in models (Hertzian, frictionless), 2 the one compiled at run time (deme_jit.h)
inline int model_class(const deme_ctx* c) {
    return c->hp.forceModel == DEME_FORCE_CUSTOM ? 2 : (c->hp.forceModel == DEME_FORCE_HERTZIAN ? 0 : 1);
}

// the stride of the staged owner records of a tile launch (TileArgs::rs16): padded by 16 bytes when that costs no workgroup per CU
// (160 KB of LDS per CU, allocated in 512-byte blocks; the kernels' registers allow four workgroups)
static uint32_t tile_record_stride(uint32_t hCap, uint32_t lCap, uint32_t tabBytes, int model) {
    const uint32_t base = tile_rec16(model);
    if (model == 2)  // (80-byte records start on 16 banks already)
        return base;
    auto groups = [&](uint32_t rs) { return std::min<uint32_t>(4u, 163840u / ((tile_lds_bytes(hCap, lCap, tabBytes, rs) + 511u) & ~511u)); };
    return groups(base + 1u) == groups(base) ? base + 1u : base;
}

// A tile launch (k_tile_forces, k_tile_step and the instances compiled at run time), described once: the list's tile structures, the
// current owners and wildcards, and the launch's shape -- the block count and the LDS bytes, sized for a largest halo of `maxHalo`
// staged owners (rounded up so that a launch configuration serves many detections).  The callers add what is their own.
struct TileLaunch {
    TileArgs a;
    unsigned nBlk;
    uint32_t ldsBytes;
};
TileLaunch tile_launch(deme_ctx* c, ContactList& L, int model, uint32_t maxHalo) {
    TileLaunch t{};
    TileArgs& ta = t.a;
    ta.owners = c->owners.as<OwnerRec>();
    ta.tInfo = L.tInfo.as<uint2>();
    ta.aStart = L.aStart.as<uint32_t>();
    ta.hList = L.hList.as<uint32_t>(), ta.hCount = L.hCount.as<uint32_t>(), ta.org = L.tileOrg.as<int64_t>();
    ta.lOff = L.lOff.as<uint16_t>(), ta.lPos = L.lPos.as<uint16_t>(), ta.lCount = L.lCount.as<uint32_t>();
    ta.wc = c->wc[c->wcCur].as<float>();
    ta.nOwners = c->nOwners;
    ta.nTiles = (c->nOwners + DEME_TILE_NB - 1) / DEME_TILE_NB;
    ta.xcdGroup = c->xcdGroup;
    ta.tileBig = L.tileBig.as<uint32_t>(), ta.bigList = L.bigList.as<uint32_t>(), ta.info = L.info.as<uint4>();
    ta.hCap = std::min<uint32_t>(DEME_TILE_HMAX, (maxHalo + 15u) & ~15u);
    ta.lCap = std::min<uint32_t>(DEME_TILE_LMAX, (L.tileMaxList + 15u) & ~15u);
    ta.nComp = c->nComp, ta.nAnal = c->nAnal, ta.nMass = c->nMassProps;
    const uint32_t tabBytes = tile_table_bytes(c->nComp, c->nMat, c->nAnal, c->nMassProps, c->dp.familyTrivial);
    ta.rs16 = tile_record_stride(ta.hCap, ta.lCap, tabBytes, model);
    ta.swz = (model != 2 && ta.rs16 == tile_rec16(model)) ? 1u : 0u;
    t.nBlk = xcd_round(ta.nTiles, ta.xcdGroup);
    t.ldsBytes = tile_lds_bytes(ta.hCap, ta.lCap, tabBytes, ta.rs16);
    return t;
}

// The general kernel (one contact per thread) of a model class, over nBlk blocks: its mesh variant (the sphere-triangle work list),
// the fast kernel of the built-in models, or the exact one.  A user model has two entry points: the mesh variant and the other.
enum class General { Mesh, Fast, Exact };
int launch_general(deme_ctx* c, int model, General which, unsigned nBlk, ForceArgs& a) {
    if (model == 2) {
        void* args[] = {&c->dp, &a};
        HIPCK(hipModuleLaunchKernel(c->customFn[which == General::Mesh ? 1 : 0], nBlk, 1, 1, DEME_FORCE_BLOCK, 1, 1, 0, c->stream, args,
                                    nullptr));
        return DEME_OK;
    }
    as_constant(model == 1, [&](auto frictionless) {
        constexpr int M = decltype(frictionless)::value ? 1 : 0;
        const dim3 g(nBlk), b(DEME_FORCE_BLOCK);
        if (which == General::Mesh)
            hipLaunchKernelGGL((k_calc_forces<M, 1>), g, b, 0, c->stream, c->dp, a);
        else if (which == General::Fast)
            hipLaunchKernelGGL((k_forces_fast<M>), g, b, 0, c->stream, c->dp, a);
        else
            hipLaunchKernelGGL((k_calc_forces<M, 0>), g, b, 0, c->stream, c->dp, a);
    });
    return DEME_OK;
}
// The tile kernels of (model class, mesh records, recording): the tiles that fit LDS, then one workgroup for each of the list's tiles
// that do not, with the same outputs (deme_tile.h).  A user model's are the same kernels compiled around its statements (deme_jit.h).
int launch_tiles(deme_ctx* c, const ContactList& L, int model, bool mesh, bool rec, TileLaunch& t) {
    const unsigned nBig = L.nBigTiles;
    if (model == 2) {
        void* args[] = {&c->dp, &t.a};
        HIPCK(hipModuleLaunchKernel(c->customTileFn[mesh ? 1 : 0], t.nBlk, 1, 1, DEME_TILE_T, 1, 1, t.ldsBytes, c->stream, args, nullptr));
        if (nBig)
            HIPCK(hipModuleLaunchKernel(c->customTileFn[mesh ? 3 : 2], nBig, 1, 1, DEME_TILE_T, 1, 1, 0, c->stream, args, nullptr));
        return DEME_OK;
    }
    as_constant(model == 1, [&](auto frictionless) {
        as_constant(mesh, [&](auto withMesh) {
            as_constant(rec, [&](auto withRec) {
                constexpr int M = decltype(frictionless)::value ? 1 : 0;
                constexpr bool MESH = decltype(withMesh)::value, REC = decltype(withRec)::value;
                hipLaunchKernelGGL((k_tile_forces<M, MESH, REC>), dim3(t.nBlk), dim3(DEME_TILE_T), t.ldsBytes, c->stream, c->dp, t.a);
                if (nBig)
                    hipLaunchKernelGGL((k_tile_forces_big<M, MESH, REC>), dim3(nBig), dim3(DEME_TILE_T), 0, c->stream, c->dp, t.a);
            });
        });
    });
    return DEME_OK;
}

// pass: -1 everything in one launch; 0 / 1 the two halves of a split step (contacts that read no ghost owner / the rest)
int launch_forces(deme_ctx* c, int pass = -1) {
    ContactList& L = c->list[c->cur];
    c->fusedPrevValid = false;
    if (c->nContacts == 0) {
        c->conValid = true;
        c->conTile = false;
        return DEME_OK;
    }
    if (c->hp.forceModel == DEME_FORCE_CUSTOM && !c->customFn[0])
        return fail(c, DEME_ERR_INVALID, "custom force model selected but none compiled (deme_compile_force_model)");
    ForceArgs a{};
    a.owners = c->owners.as<OwnerRec>();
    a.spheres = c->spheres.as<SphereRec>();
    a.keys = c->keysSorted[c->keysCur].as<uint64_t>();
    a.info = L.info.as<uint4>();
    a.wc = c->wc[c->wcCur].as<float>();
    a.conA4 = c->conA4.as<float4>(), a.conA2 = c->conA2.as<float2>();
    a.conB4 = c->conB4.as<float4>(), a.conB2 = c->conB2.as<float2>();
    a.aSum = c->aSum.as<float4>();
    a.aStart = L.aStart.as<uint32_t>();
    a.smList = L.smList.as<uint32_t>();
    a.nSM = L.nSM;
    for (int k = 0; k < 8; k++) {
        a.ownerWc[k] = c->userWc[0][k].as<float>();
        a.geoWcSph[k] = c->userWc[1][k].as<float>();
        a.geoWcTri[k] = c->userWc[2][k].as<float>();
        a.geoWcAnal[k] = c->userWc[3][k].as<float>();
    }
    if (pass >= 0 && c->hasGhosts && L.cDefer.p) {
        a.cDefer = L.cDefer.as<uint8_t>();
        a.blockMode = L.blockMode.as<uint32_t>();
        a.pass = (uint32_t)pass;
    }
    if (c->record) {  // (on the tile path these serve the mesh variant of the general kernel, which records its own contacts)
        a.recForce = c->rec[0].as<float>(), a.recTorque = c->rec[1].as<float>(), a.recCPA = c->rec[2].as<float>(),
        a.recCPB = c->rec[3].as<float>();
    }
    a.nContacts = (uint32_t)c->nContacts;
    a.timeElapsed = (float)c->timeElapsed;
    a.xcdGroup = c->xcdGroup;
    const bool fastMode = c->arith == DEME_ARITH_FAST;
    a.world = fastMode ? 1u : 0u;
    // The owner tiles (deme_tile.h) serve the fast mode: the built-in models with or without contact recording (REC instances), a
    // user model when it is not recording.  Everything else -- the exact mode, a recording user model (the reference's body-frame
    // vocabulary), a list without tile structures -- runs the general kernel, the fast one where there is one and nothing is recorded.
    const int model = model_class(c);
    const bool tiles = fastMode && L.tileActive && (model != 2 || (!c->record && c->customTileFn[0]));
    if (tiles) {
        if (L.fusedList && !L.fusedChecked)
            resolve_heavy_counts(c, L);
    } else {
        c->conTile = false;
        if (int rc = ensure_legacy_lists(c))  // (a list with tile structures that is evaluated by the other kernels after all: recording switched on, ...)
            return rc;
    }
    ScopedTimer tm(c, "calc_forces");
    // sphere-triangle contacts: the mesh variant of the general kernel, ahead of the kernels that take its records in (the tiles read
    // them, the hot variant folds its A-side records into the in-block sums).  They read no ghost owner -- meshes are replicated,
    // not ghosted --: all of them go with pass 0.
    const bool mesh = c->nTri > 0 && L.nSM > 0;
    if (mesh && pass != 1)
        if (int rc = launch_general(c, model, General::Mesh, grid_for(L.nSM, DEME_FORCE_BLOCK), a))
            return rc;
    if (tiles) {
        TileLaunch t = tile_launch(c, L, model, L.tileMaxHalo);
        TileArgs& ta = t.a;
        ta.tSum = a.aSum;
        ta.rec32 = c->rec32.as<float4>(), ta.rankC = L.rankC.as<uint32_t>();
        ta.keys = a.keys, ta.timeElapsed = a.timeElapsed;
        for (int k = 0; k < 8; k++)
            ta.ownerWc[k] = a.ownerWc[k], ta.geoWcSph[k] = a.geoWcSph[k], ta.geoWcAnal[k] = a.geoWcAnal[k];
        if (c->record)
            for (int k = 0; k < 4; k++)
                ta.rec[k] = c->rec[k].as<float>();
        if (mesh)
            ta.conA4 = a.conA4, ta.conA2 = a.conA2, ta.conB4 = a.conB4, ta.conB2 = a.conB2;
        if (pass >= 0 && c->hasGhosts) {
            ta.tileMode = L.tileMode.as<uint32_t>();
            ta.pass = (uint32_t)pass;
        }
        if (int rc = launch_tiles(c, L, model, mesh, c->record, t))
            return rc;
    } else {
        const General which = (fastMode && model != 2 && !c->record) ? General::Fast : General::Exact;
        if (int rc = launch_general(c, model, which, xcd_round(grid_for(a.nContacts, DEME_FORCE_BLOCK), a.xcdGroup), a))
            return rc;
    }
    c->conValid = true;
    c->conTile = tiles;
    return DEME_OK;
}

// accelerations a script added for the coming step (deme_add_owner_acc): both copies to zero ...
int zero_next_acc(deme_ctx* c) {
    std::fill(c->hNextAcc.begin(), c->hNextAcc.end(), AccRec{});
    HIPCK(hipMemsetAsync(c->nextAcc.p, 0, (size_t)c->nOwners * sizeof(AccRec), c->stream));
    return DEME_OK;
}
// ... which the step that has read them does: they hold for one step only (cleanUpAcc clears the flag when it honours it,
// DEMPrepForceKernels.cu:14-31)
int clear_next_acc(deme_ctx* c) {
    if (!c->nextAccPending)
        return DEME_OK;
    c->nextAccPending = false;
    return zero_next_acc(c);
}
// the step counter and the clock (on their own for deme_integrate: a staged caller schedules its own detections)
void advance_clock(deme_ctx* c) {
    c->nSteps++;
    c->timeElapsed += (double)c->hp.h;
}
// the end of a step of deme_step and its kin: the list is a step older, and the halo stream may pack the owners just integrated
int finish_step(deme_ctx* c) {
    c->stepsSinceCD++;
    advance_clock(c);
    if (c->evStepDone)
        HIPCK(hipEventRecord(c->evStepDone, c->stream));
    return DEME_OK;
}

// The whole step in one launch (deme_tile_step.h).  dry: replay the force evaluation of the step just taken on the buffers of its
// start and leave a / alpha (state downloads).
bool fused_ready(deme_ctx* c) {
    ContactList& L = c->list[c->cur];
    if (!L.fusedList || !L.tileActive || c->arith != DEME_ARITH_FAST || c->record || c->hp.forceModel == DEME_FORCE_CUSTOM ||
        c->prescFn || c->rulesFn || c->nContacts == 0)
        return false;
    if (!L.fusedChecked)
        resolve_heavy_counts(c, L);
    return L.fusedList && L.nHeavyFree == 0;
}
int launch_fused_step(deme_ctx* c, bool dry) {
    ContactList& L = c->list[c->cur];
    const int model = c->hp.forceModel == DEME_FORCE_HERTZIAN ? 0 : 1;  // (never a user model: fused_ready)
    const TileLaunch t = tile_launch(c, L, model, L.tileMaxHaloIn);  // (the halos with the incoming contacts' owners: k_tile_incoming)
    StepArgs sa{};
    sa.t = t.a;
    const int cur = dry ? (c->wcCur ^ 1) : c->wcCur;  // (dry: the step is over, the names are swapped already)
    sa.t.owners = dry ? c->ownersNext.as<OwnerRec>() : c->owners.as<OwnerRec>();
    sa.t.wc = c->wc[cur].as<float>();
    sa.t.hCount = c->hCountIn.as<uint32_t>();
    sa.ownersNext = dry ? c->owners.as<OwnerRec>() : c->ownersNext.as<OwnerRec>();
    sa.wcNext = c->wc[cur ^ 1].as<float>();
    sa.tInfoIn = c->tInfoIn.as<uint2>(), sa.inContact = c->inContact.as<uint32_t>(), sa.inStart = c->inStart.as<uint32_t>();
    sa.acc = c->acc.as<AccRec>();
    sa.nextAcc = (!dry && c->nextAccPending) ? c->nextAcc.as<AccRec>() : nullptr;
    sa.dry = dry ? 1u : 0u;
    {
        ScopedTimer tm(c, dry ? "fused_replay" : "calc_forces");
        as_constant(model == 1, [&](auto frictionless) {
            hipLaunchKernelGGL((k_tile_step<decltype(frictionless)::value ? 1 : 0>), dim3(t.nBlk), dim3(DEME_TILE_T), t.ldsBytes, c->stream,
                               c->dp, sa);
        });
    }
    if (dry)
        return DEME_OK;
    std::swap(c->owners, c->ownersNext);
    c->wcCur ^= 1;
    if (int rc = clear_next_acc(c))
        return rc;
    c->conValid = false, c->conTile = false;
    c->fusedPrevValid = true;
    c->nFusedSteps++;
    return finish_step(c);
}

// owners of prescribed families (rebuilt when families were uploaded); host-side: this is a set-up path
int rebuild_presc_list(deme_ctx* c) {
    c->prescDirty = false;
    c->nPresc = 0;
    if (!c->prescFn)
        return DEME_OK;
    std::vector<uint32_t> list, slot(c->nOwners, 0u);
    if (c->rulesFn) {  // families change on the device: every owner may become prescribed, so every owner gets a record
        list.resize(c->nOwners);
        for (uint32_t o = 0; o < c->nOwners; o++)
            list[o] = slot[o] = o;
    } else {
        std::vector<OwnerRec> h(c->nOwners);
        HIPCK(hipMemcpyAsync(h.data(), c->owners.p, (size_t)c->nOwners * sizeof(OwnerRec), hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        for (uint32_t o = 0; o < c->nOwners; o++)
            if (c->hostFamFlags[h[o].family & 255u] & DEME_FAMILY_PRESCRIBED) {
                slot[o] = (uint32_t)list.size();
                list.push_back(o);
            }
    }
    c->nPresc = (uint32_t)list.size();
    if (int rc = ensure(c, c->prescList, std::max<size_t>(list.size(), 1) * 4))
        return rc;
    if (int rc = ensure(c, c->prescSlot, std::max<size_t>(c->nOwners, 1) * 4))
        return rc;
    if (int rc = ensure(c, c->prescRec, std::max<size_t>(list.size(), 1) * sizeof(PrescRec)))
        return rc;
    if (!list.empty())
        HIPCK(hipMemcpyAsync(c->prescList.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(c->prescSlot.p, slot.data(), slot.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

// Where k_integrate finds an owner's a / alpha -- stored in `acc` by a full reduction, or gathered by itself from the contributions
// (heavy owners excepted: launch_reduce_heavy has stored theirs) -- and which owners it moves.  NotWaiting (slab group, one
// evaluation per cross-cut contact): the owners that wait for a reverse share are left out (GatherArgs::revPhase) and the step is
// not over; launch_integrate_later integrates them once the share has arrived.
enum class AccFrom { Stored, Contributions };
enum class Owners { All, NotWaiting };
int launch_integrate(deme_ctx* c, AccFrom from, Owners who = Owners::All) {
    ContactList& L = c->list[c->cur];
    ScopedTimer tm(c, "integrate");
    PrescArgs pa{nullptr, nullptr};
    if (c->prescFn) {
        if (c->prescDirty)
            if (int rc = rebuild_presc_list(c))
                return rc;
        if (c->nPresc) {
            const OwnerRec* ow = c->owners.as<OwnerRec>();
            const uint32_t* list = c->prescList.as<uint32_t>();
            PrescRec* rec = c->prescRec.as<PrescRec>();
            uint32_t n = c->nPresc;
            float t = (float)c->timeElapsed;
            void* args[] = {&c->dp, &ow, &list, &n, &rec, &t};
            HIPCK(hipModuleLaunchKernel(c->prescFn, grid_for(n), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
            pa.rec = rec;
            pa.slot = c->prescSlot.as<uint32_t>();
        }
    }
    if (from == AccFrom::Contributions) {
        if (L.heavyOverflow)
            return c->lastStatus;
        GatherArgs ga = gather_args(c);
        ga.revPhase = who == Owners::NotWaiting ? 1u : 0u;
        if (c->nOwners)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
        hipLaunchKernelGGL(k_integrate<true>, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->dp,
                           c->owners.as<OwnerRec>(), c->acc.as<AccRec>(), ga, pa);
    } else {
        if (c->nOwners)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
        hipLaunchKernelGGL(k_integrate<false>, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->dp,
                           c->owners.as<OwnerRec>(), c->acc.as<AccRec>(), gather_args(c), pa);
    }
    c->laterPa = pa;
    if (who == Owners::NotWaiting)
        return DEME_OK;
    return clear_next_acc(c);
}
int launch_integrate_later(deme_ctx* c, const uint32_t* ids, uint32_t n) {
    if (n) {
        ScopedTimer tm(c, "integrate_later");
        hipLaunchKernelGGL(k_integrate_list, dim3(grid_for(n)), dim3(256), 0, c->stream, c->dp, c->owners.as<OwnerRec>(),
                           c->acc.as<AccRec>(), gather_args(c), c->laterPa, ids, n);
    }
    return clear_next_acc(c);
}

// a/alpha of every owner from the current contributions (stand-alone force pass and state downloads)
void launch_full_reduction(deme_ctx* c) {
    if (c->nOwners)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
    hipLaunchKernelGGL(k_gather_acc, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->dp, gather_args(c),
                       c->owners.as<OwnerRec>(), c->acc.as<AccRec>());
    launch_reduce_heavy(c, false);
}

}  // namespace

#include "deme_order.inc"

// ================================================================================================
extern "C" {

const char* deme_version(void) { return "deme_hip 0.1 (gfx950)"; }

int deme_ctx_create(int device, deme_ctx** out) {
    if (!out)
        return DEME_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device >= n)
        return DEME_ERR_HIP;  // reference: DEMSolver construction throws when no device (GpuManager.cpp:64-68)
    if (hipSetDevice(device) != hipSuccess)
        return DEME_ERR_HIP;
    deme_ctx* c = new deme_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return DEME_ERR_HIP;
    }
    if (ensure(c, c->ctr, sizeof(DetectBlock)) || ensure(c, c->scanTmp, 1 << 20)) {
        delete c;
        return DEME_ERR_HIP;
    }
    hipMemsetAsync(c->ctr.p, 0, sizeof(DetectBlock), c->stream);
    if (hipHostMalloc((void**)&c->pin, PIN_BYTES, hipHostMallocDefault) != hipSuccess) {
        deme_ctx_destroy(c);
        return DEME_ERR_HIP;
    }
    if (const char* e = getenv("DEME_ARITH"))  // process-wide default of deme_set_arith_mode ("exact" / "fast")
        c->arith = (strcmp(e, "exact") == 0) ? DEME_ARITH_EXACT : DEME_ARITH_FAST;
    if (const char* e = getenv("DEME_XCD_GROUP"))  // tuning knob (profiles/): see force_block_id
        c->xcdGroup = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("DEME_SPIN_SYNC"))
        c->spinSync = atoi(e);
    if (const char* e = getenv("DEME_KEY_SEG_MIN"))  // tests lower it to put small scenes through the segmented arena; 0 = one segment always
        c->keySegMin = (size_t)std::max(0ll, atoll(e));
    *out = c;
    return DEME_OK;
}

void deme_ctx_destroy(deme_ctx* c) {
    if (!c)
        return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (auto e : c->eventPool)
        hipEventDestroy(e);
    for (hipModule_t m : {c->customMod, c->prescMod, c->rulesMod})
        if (m)
            (void)hipModuleUnload(m);
    for (hipModule_t m : c->regionMod)
        if (m)
            (void)hipModuleUnload(m);
    for (hipEvent_t e : {c->evDet0, c->evDet1, c->evWin0, c->evWin1})
        if (e)
            hipEventDestroy(e);
    if (c->haloStream) {
        hipStreamSynchronize(c->haloStream);
        hipEventDestroy(c->evStepDone);
        hipEventDestroy(c->evHaloDone);
        hipStreamDestroy(c->haloStream);
    }
    if (c->pin)
        hipHostFree(c->pin);
    for (ContactList& l : c->list)
        for (DevBuf* b : l.buffers())
            if (b->p)
                hipFree(b->p);
    if (c->hrEvent)
        hipEventDestroy(c->hrEvent);
    if (c->detStream) {
        hipStreamSynchronize(c->detStream);
        hipEventDestroy(c->evSnap);
        hipEventDestroy(c->evP1);
        hipStreamDestroy(c->detStream);
    }
    DevBuf* all[] = {&c->hCountIn, &c->ownersNext, &c->recContact, &c->inCnt, &c->inStart, &c->tInfoIn, &c->inContact,
                     &c->sphFam, &c->dO2E, &c->dS2E, &c->rec32, &c->revSlot, &c->nextAcc, &c->binStat, &c->volumes,
                     &c->persistKeys, &c->owners, &c->spheres, &c->acc, &c->conA4, &c->conA2, &c->conB4, &c->conB2, &c->aSum,
                     &c->prescList, &c->prescSlot, &c->prescRec, &c->tris, &c->triWorld, &c->triLo, &c->triHi, &c->triCounts,
                     &c->triOffsets, &c->triKeys[0], &c->triKeys[1], &c->triVals[0], &c->triVals[1], &c->comp, &c->massProps,
                     &c->anal, &c->matPair, &c->E, &c->nu, &c->CoR, &c->mu, &c->Crr, &c->famMasks, &c->famExtra, &c->famFlags,
                     &c->geo, &c->binLo, &c->binN, &c->binPartial, &c->incKeys[0], &c->incKeys[1], &c->incVals[0],
                     &c->incVals[1], &c->keysRaw, &c->keysSorted[0], &c->keysSorted[1], &c->wc[0], &c->wc[1], &c->ctr,
                     &c->scanTmp, &c->sortTmp, &c->rec[0], &c->rec[1], &c->rec[2], &c->rec[3], &c->stage, &c->sharedIds,
                     &c->sharedBuf, &c->keysMid, &c->ownersSnap, &c->rsMark, &c->rsKeys[0], &c->rsKeys[1], &c->rsRuns,
                     &c->rsUKeys, &c->rsIdx, &c->rsOldR, &c->rsUses, &c->rsRemap, &c->qMark, &c->qHits, &c->qRecs, &c->qCtr, &c->qState,
                     &c->ciMask, &c->ciCounts, &c->ciPartial, &c->ciOut, &c->segTmp, &c->segPartial, &c->tlForce, &c->tlCount, &c->twAcc, &c->twRows, &c->twOut,
                     &c->fiCellOf, &c->fiOut, &c->clParent, &c->clLabel, &c->clSize, &c->clFlag, &c->clRank, &c->clStat, &c->clTable,
                     &c->clCtl, &c->clPairs};
    for (DevBuf* b : all)
        if (b->p)
            hipFree(b->p);
    for (SegPairs* p : {&c->tlPairs, &c->fiOwn, &c->fiSide, &c->clSel})
        for (DevBuf* b : {&p->key[0], &p->key[1], &p->val[0], &p->val[1]})
            if (b->p)
                hipFree(b->p);
    for (auto& kind : c->userWc)
        for (auto& b : kind)
            if (b.p)
                hipFree(b.p);
    if (c->ownStream && c->stream)
        hipStreamDestroy(c->stream);
    delete c;
}

const char* deme_last_error(const deme_ctx* c) { return c ? c->err.c_str() : "null context"; }

int deme_ctx_set_stream(deme_ctx* c, void* s) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    HIPCK(hipStreamSynchronize(c->stream));
    if (s) {
        if (c->ownStream)
            hipStreamDestroy(c->stream);
        c->stream = (hipStream_t)s;
        c->ownStream = false;
    } else if (!c->ownStream) {
        HIPCK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->ownStream = true;
    }
    return DEME_OK;
}

int deme_set_arith_mode(deme_ctx* c, int mode) {
    if (!c || (mode != DEME_ARITH_FAST && mode != DEME_ARITH_EXACT))
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    if (mode != c->arith) {
        HIPCK(hipStreamSynchronize(c->stream));  // (an asynchronous detection cycle ends inside deme_step: nothing is in flight beside the stream)
        c->arith = mode;
        c->conValid = false;  // stored contributions are in the other mode's units
        if (mode == DEME_ARITH_EXACT) {
            // The exact mode's contract is bit-identity with the oracle, which sums an owner's contributions in the CALLER's order:
            // a context the engine had reordered goes back to that order (deme_order.inc: order_restore) and stays there.
            c->orderEligible = false, c->orderRenewDue = false;
            if (c->permuted && c->haveScene)
                if (int rc = order_restore(c))
                    return rc;
        } else if (c->haveScene && c->orderStructOK) {  // back in the fast mode: the next lock-step detection may reorder again
            c->orderEligible = true;
            c->orderRenewDue = true;
        }
    }
    return DEME_OK;
}
int deme_get_arith_mode(const deme_ctx* c) { return c ? c->arith : -1; }

int deme_force_kernel_name(const deme_ctx* c, char* name, size_t cap, uint32_t* tileMaxHalo, uint32_t* tileMaxList) {
    if (!c || !name || !cap)
        return DEME_ERR_INVALID;
    const ContactList& L = c->list[c->cur];
    const int m = c->hp.forceModel == DEME_FORCE_HERTZIAN ? 0 : 1;
    const bool fastKernel = c->arith == DEME_ARITH_FAST && c->hp.forceModel != DEME_FORCE_CUSTOM;
    if (c->fusedPrevValid && L.fusedList && L.tileActive)  // the last step went through the one-kernel step (deme_tile_step.h)
        snprintf(name, cap, "k_tile_step<%d>", m);
    else if (c->hp.forceModel == DEME_FORCE_CUSTOM && c->arith == DEME_ARITH_FAST && !c->record && c->customTileFn[0] && L.tileActive)
        snprintf(name, cap, "deme_custom_tile<%s>", (c->nTri > 0 && L.nSM > 0) ? "true" : "false");
    else if (c->hp.forceModel == DEME_FORCE_CUSTOM)
        snprintf(name, cap, "deme_custom_forces_ss");
    else if (fastKernel && L.tileActive)
        snprintf(name, cap, "k_tile_forces<%d, %s>", m, (c->nTri > 0 && L.nSM > 0) ? "true" : "false");
    else if (fastKernel && !c->record)
        snprintf(name, cap, "k_forces_fast<%d>", m);
    else
        snprintf(name, cap, "k_calc_forces<%d, 0>", m);
    if (tileMaxHalo)
        *tileMaxHalo = L.tileMaxHalo;
    if (tileMaxList)
        *tileMaxList = L.tileMaxList;
    return DEME_OK;
}

int deme_tile_stats(const deme_ctx* c, uint32_t out[4]) {
    if (!c || !out)
        return DEME_ERR_INVALID;
    const ContactList& L = c->list[c->cur];
    out[0] = L.tileActive ? (c->nOwners + DEME_TILE_NB - 1) / DEME_TILE_NB : 0u;
    out[1] = L.tileActive ? L.nBigTiles : 0u;
    out[2] = L.tileMaxHalo, out[3] = L.tileMaxList;
    return DEME_OK;
}
int deme_heavy_owners(deme_ctx* c, uint32_t out[2]) {
    if (!c || !out)
        return DEME_ERR_INVALID;
    ContactList& L = c->list[c->cur];
    resolve_heavy_counts(c, L);
    out[0] = L.nHeavy, out[1] = L.nHeavyFree;
    return DEME_OK;
}
int deme_set_tile_policy(deme_ctx* c, uint32_t minContactsPerTileCustom) {
    if (!c)
        return DEME_ERR_INVALID;
    c->tileMinContactsCustom = minContactsPerTileCustom;
    c->listStale = true;
    return DEME_OK;
}
int deme_set_fused_step(deme_ctx* c, int on) {
    if (!c)
        return DEME_ERR_INVALID;
    c->fusedEnable = on == 2 ? 2 : (on ? 1 : 0);
    c->listStale = true;
    return DEME_OK;
}
int deme_get_order(const deme_ctx* c, int* reordered, double spread[2]) {
    if (!c)
        return DEME_ERR_INVALID;
    if (reordered)
        *reordered = c->permuted ? 1 : 0;
    if (spread)
        spread[0] = c->orderSpread[0], spread[1] = c->orderSpread[1];
    return DEME_OK;
}
int deme_order_renewals(const deme_ctx* c, uint64_t* n) {
    if (!c || !n)
        return DEME_ERR_INVALID;
    *n = c->nOrderRenewals;
    return DEME_OK;
}
int deme_renew_order(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    if (!c->orderEligible || c->arith != DEME_ARITH_FAST)
        return fail(c, DEME_ERR_INVALID, "this scene keeps the caller's order (exact arithmetic mode, ghosts, or reordering switched off)");
    // (the re-keyed list is left as the SEED of the next detection -- order_apply: deme_calc_forces refuses it, a step detects first,
    // the history map and contact records are not offered from it, the sphere geometry is recomputed by that detection)
    return order_renew(c);
}
int deme_order_probe(const DemeParams* p, size_t nClumps, const uint64_t* voxelID, const uint16_t* locX, const uint16_t* locY,
                     const uint16_t* locZ, uint32_t* order, double spread[2]) {
    if (!p || !voxelID || !locX || !locY || !locZ || !spread || !(p->binSize > 0) || !(p->l > 0))
        return DEME_ERR_INVALID;
    std::vector<uint32_t> ord;
    order_compute(*p, nClumps, voxelID, locX, locY, locZ, ord, spread);
    if (order)
        memcpy(order, ord.data(), nClumps * 4);
    return DEME_OK;
}
int deme_set_reorder(deme_ctx* c, int enable) {
    if (!c)
        return DEME_ERR_INVALID;
    c->reorderEnable = enable ? 1 : 0;
    return DEME_OK;
}

int deme_sync(deme_ctx* c) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_set_params(deme_ctx* c, const DemeParams* p) {
    if (!c || !p)
        return DEME_ERR_INVALID;
    if (p->nContactWildcards > DEME_MAX_WILDCARD_NUM)
        return fail(c, DEME_ERR_INVALID, "at most %d contact wildcards", DEME_MAX_WILDCARD_NUM);
    if (p->forceModel == DEME_FORCE_HERTZIAN && p->nContactWildcards != 4)
        return fail(c, DEME_ERR_INVALID, "the Hertzian model carries 4 contact wildcards");
    if (c->haveParams && c->hp.nContactWildcards != p->nContactWildcards && c->haveList)
        return fail(c, DEME_ERR_INVALID, "the wildcard count cannot change once a contact list exists");
    if (p->nbX == 0 || p->nbY == 0 || p->nbZ == 0 || !(p->binSize > 0) || !(p->voxelSize > 0) || !(p->l > 0))
        return fail(c, DEME_ERR_INVALID, "bin / voxel sizing is incomplete");
    c->hp = *p;
    c->timeElapsed = p->timeElapsed;
    c->haveParams = true;
    refresh_dev_params(c);
    return DEME_OK;
}

// ---- the scratch a scene of nO owners / nS spheres needs: ONE statement of it, used by deme_upload_scene and by the slab migration
// (deme_migrate_host.inc), whose slabs change their counts.  (A second, shorter list in the migration once missed sphFam: a slab that
// had grown wrote its ghosts' family words past the end of the buffer.)
static int owner_scratch_for_counts(deme_ctx* c, size_t nO) {
    if (int rc = ensure(c, c->acc, std::max<size_t>(nO, 1) * sizeof(AccRec)))
        return rc;
    if (ensure(c, c->ownersNext, std::max<size_t>(nO, 1) * sizeof(OwnerRec)) || ensure(c, c->inCnt, (nO + 2) * 4) || ensure(c, c->inStart, (nO + 2) * 4))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->acc.p, 0, c->acc.bytes, c->stream));
    ContactList& L = c->list[c->cur];
    const size_t nTiles = (nO + DEME_TILE_NB - 1) / DEME_TILE_NB + 1;
    if (ensure(c, c->aSum, (nO + 1) * 32) || ensure(c, c->hCountIn, nTiles * 4))
        return c->lastStatus;
    if (int rc = size_list_per_owner(c, L, nO))
        return rc;
    L.invalidate();  // (what it holds was built for the old owners)
    c->fusedPrevValid = c->conTile = false;
    HIPCK(hipMemsetAsync(L.hCount.p, 0, L.hCount.bytes, c->stream));
    HIPCK(hipMemsetAsync(L.aStart.p, 0, L.aStart.bytes, c->stream));
    HIPCK(hipMemsetAsync(L.bStart.p, 0, L.bStart.bytes, c->stream));
    HIPCK(hipMemsetAsync(L.heavy.p, 0, L.heavy.bytes, c->stream));
    HIPCK(hipMemsetAsync(L.fixedFlag.p, 0, L.fixedFlag.bytes, c->stream));
    HIPCK(hipMemsetAsync(L.rangeCtr.p, 0, sizeof(RangeCounters), c->stream));
    return DEME_OK;
}
static int sphere_scratch_for_counts(deme_ctx* c, size_t nS) {
    if (ensure(c, c->sphFam, std::max<size_t>(nS, 1) * 2) || ensure(c, c->geo, std::max<size_t>(nS, 1) * sizeof(GeoRec)) ||
        ensure(c, c->binLo, std::max<size_t>(nS, 1) * 16) || ensure(c, c->binN, std::max<size_t>(nS, 1) * 8) ||
        ensure(c, c->binPartial, (size_t)grid_for(std::max<size_t>(nS, 1)) * 4))  // one sum per workgroup of k_sphere_prep
        return c->lastStatus;
    return DEME_OK;
}

namespace {
int tri_wear_clear(deme_ctx* c);  // (mesh wear, below: a scene with another triangle count clears the sums)
}

int deme_upload_scene(deme_ctx* c, const DemeScene* s) {
    if (!c || !s)
        return DEME_ERR_INVALID;
    if (!c->haveParams)
        return fail(c, DEME_ERR_INVALID, "call deme_set_params before deme_upload_scene");
    if (s->nSpheres >= (1u << 31))
        return fail(c, DEME_ERR_INVALID, "sphere ids must fit 31 bits");
    if (s->nOwners >= (1u << 30))
        return fail(c, DEME_ERR_INVALID, "owner ids must fit 30 bits");
    // Spheres are clump-major with ascending owners (kT.cpp:766-797): the A / B roles of a pair follow the owner
    // numbers (= the reference's "smaller sphere id first" exactly under this contract), and seeded history and persistent marks
    // are canonicalised by sphere id.
    for (size_t i = 1; i < s->nSpheres; i++)
        if (s->ownerClumpBody[i] < s->ownerClumpBody[i - 1])
            return fail(c, DEME_ERR_INVALID, "deme_upload_scene: spheres must be clump-major with ascending owners (sphere %zu belongs to owner %u, "
                        "sphere %zu to owner %u)", i - 1, s->ownerClumpBody[i - 1], i, s->ownerClumpBody[i]);
    hipSetDevice(c->device);
    c->nOwners = s->nOwners, c->nOwnerClumps = s->nOwnerClumps, c->nSpheres = s->nSpheres, c->nAnal = s->nAnal;
    c->nextAccPending = false;  // per-owner records of the previous scene do not carry over
    c->hNextAcc.clear();
    c->nMat = s->nMat, c->nComp = s->nComp, c->nMassProps = s->nMassProps;
    const size_t nO = s->nOwners, nS = s->nSpheres;
    // (persistent marks are kept in the engine's ids: they cross a re-upload in the caller's)
    for (auto& k : c->hPersist)
        k = order_key_out(c, k);
    // the engine's own order of clumps and spheres (deme_order.inc): slot k holds the caller's owner o2e(k)
    c->permuted = order_decide(c, s);
    c->viewSerial = ~0ull;
    c->orderRenewDue = false, c->orderBaseHalo = 0;
    auto o2e = [&](size_t k) { return c->permuted ? (size_t)c->hO2E[k] : k; };
    // owners
    std::vector<OwnerRec> ho(nO);
    for (size_t k = 0; k < nO; k++) {
        const size_t i = o2e(k);
        OwnerRec& r = ho[k];
        r.voxelID = s->voxelID[i];
        r.locX = s->locX[i], r.locY = s->locY[i], r.locZ = s->locZ[i];
        r.inertiaOff = s->inertiaPropOffsets ? s->inertiaPropOffsets[i] : 0;
        r.qw = s->oriQw ? s->oriQw[i] : 1.f, r.qx = s->oriQx ? s->oriQx[i] : 0.f, r.qy = s->oriQy ? s->oriQy[i] : 0.f,
        r.qz = s->oriQz ? s->oriQz[i] : 0.f;
        r.vx = s->vX ? s->vX[i] : 0.f, r.vy = s->vY ? s->vY[i] : 0.f, r.vz = s->vZ ? s->vZ[i] : 0.f;
        r.wx = s->omgBarX ? s->omgBarX[i] : 0.f, r.wy = s->omgBarY ? s->omgBarY[i] : 0.f,
        r.wz = s->omgBarZ ? s->omgBarZ[i] : 0.f;
        r.family = s->familyID ? s->familyID[i] : 0;
        r.margin = 0.f;
    }
    if (int rc = upload(c, c->owners, ho.data(), nO))
        return rc;
    if (int rc = owner_scratch_for_counts(c, nO))
        return rc;
    c->conValid = false;
    // spheres
    std::vector<SphereRec> hs(nS);
    for (size_t k = 0; k < nS; k++) {
        const size_t i = c->permuted ? (size_t)c->hS2E[k] : k;
        hs[k].owner = order_owner_in(c, s->ownerClumpBody[i]);
        hs[k].comp = s->clumpComponentOffset[i];
        hs[k].mat = s->sphereMaterialOffset ? s->sphereMaterialOffset[i] : 0;
    }
    if (int rc = upload(c, c->spheres, hs.data(), nS))
        return rc;
    // tables
    std::vector<float4> hc(s->nComp), hm(s->nMassProps);
    for (uint32_t i = 0; i < s->nComp; i++)
        hc[i] = make_float4(s->CDRelPosX[i], s->CDRelPosY[i], s->CDRelPosZ[i], s->Radii[i]);
    for (uint32_t i = 0; i < s->nMassProps; i++)
        hm[i] = make_float4(s->MassProperties[i], s->moiX[i], s->moiY[i], s->moiZ[i]);
    if (int rc = upload(c, c->comp, hc.data(), hc.size()))
        return rc;
    c->hComp = hc;
    c->nTemplateComps = s->nComp;
    if (int rc = upload(c, c->massProps, hm.data(), hm.size()))
        return rc;
    std::vector<AnalObj> ha(s->nAnal);
    c->hObjType.assign(s->nAnal, 0);
    for (uint32_t i = 0; i < s->nAnal; i++) {
        AnalObj& a = ha[i];
        memset(&a, 0, sizeof(a));
        a.relx = s->objRelPosX[i], a.rely = s->objRelPosY[i], a.relz = s->objRelPosZ[i];
        a.rotx = s->objRotX[i], a.roty = s->objRotY[i], a.rotz = s->objRotZ[i];
        a.size1 = s->objSize1 ? s->objSize1[i] : 0.f, a.size2 = s->objSize2 ? s->objSize2[i] : 0.f,
        a.size3 = s->objSize3 ? s->objSize3[i] : 0.f;
        a.normal = s->objNormal ? s->objNormal[i] : 1.f;
        a.mass = s->objMass ? s->objMass[i] : 1e6f;
        a.owner = s->objOwner[i];
        a.type = s->objType[i];
        a.mat = s->objMaterial ? s->objMaterial[i] : 0;
        c->hObjType[i] = s->objType[i];
    }
    if (int rc = upload(c, c->anal, ha.data(), ha.size()))
        return rc;
    c->mt.nMat = s->nMat;
    c->mt.E.assign(s->E, s->E + s->nMat);
    c->mt.nu.assign(s->nu, s->nu + s->nMat);
    if (s->CoR) c->mt.CoR.assign(s->CoR, s->CoR + (size_t)s->nMat * s->nMat);
    if (s->mu) c->mt.mu.assign(s->mu, s->mu + (size_t)s->nMat * s->nMat);
    if (s->Crr) c->mt.Crr.assign(s->Crr, s->Crr + (size_t)s->nMat * s->nMat);
    std::vector<MatPair> hp;
    build_mat_pairs(s, hp);
    if (int rc = upload(c, c->matPair, hp.data(), hp.size()))
        return rc;
    const size_t nM = s->nMat;
    if (upload(c, c->E, s->E, nM) || upload(c, c->nu, s->nu, nM) || upload(c, c->CoR, s->CoR, nM * nM) ||
        upload(c, c->mu, s->mu, nM * nM) || upload(c, c->Crr, s->Crr, nM * nM))
        return c->lastStatus;
    if (upload(c, c->famMasks, s->familyMasks, (size_t)DEME_FAMILY_MASK_ENTRIES) ||
        upload(c, c->famExtra, s->familyExtraMarginSize, (size_t)DEME_NUM_FAMILIES) ||
        upload(c, c->famFlags, s->familyFlags, (size_t)DEME_NUM_FAMILIES))
        return c->lastStatus;
    memset(c->hostFamFlags, 0, sizeof(c->hostFamFlags));
    if (s->familyFlags)
        memcpy(c->hostFamFlags, s->familyFlags, DEME_NUM_FAMILIES);
    c->hasGhosts = false;
    c->hShared.clear();
    {   // per-owner flags: bit 0 ghost copy, bit 1 replicated free owner.  Always written: a context may be given a new scene
        std::vector<uint8_t> fl(std::max<size_t>(nO, 16), 0);
        if (s->ownerGhost)
            for (size_t i = 0; i < nO; i++) {
                fl[i] = s->ownerGhost[i] & 3u;
                c->hasGhosts = c->hasGhosts || (fl[i] & 1u);
                if (fl[i] & 2u)
                    c->hShared.push_back((uint32_t)i);
            }
        if (int rc = ensure(c, c->stage, fl.size()))
            return rc;
        HIPCK(hipMemcpyAsync(c->stage.p, fl.data(), nO, hipMemcpyHostToDevice, c->stream));
        if (nO)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
        hipLaunchKernelGGL(k_set_ghost_bits, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, c->owners.as<OwnerRec>(),
                           c->stage.as<uint8_t>());
        HIPCK(hipStreamSynchronize(c->stream));  // fl is a local
        if (!c->hShared.empty())
            if (int rc = upload(c, c->sharedIds, c->hShared.data(), c->hShared.size()))
                return rc;
    }
    c->prescDirty = true;
    bool trivial = true;
    if (s->familyMasks)
        for (size_t i = 0; i < DEME_FAMILY_MASK_ENTRIES && trivial; i++)
            trivial = s->familyMasks[i] == 0;
    if (s->familyExtraMarginSize)
        for (size_t i = 0; i < DEME_NUM_FAMILIES && trivial; i++)
            trivial = s->familyExtraMarginSize[i] == 0.f;
    c->dp.familyTrivial = trivial ? 1u : 0u;
    if (c->pairsOnce) {  // the fresh owners carry no passive marks and the reaction slots were sized for the old scene: the group
                         // sets the mode up again before its next step (rev_setup_slab), until then this context evaluates both ways
        c->pairsOnce = false;
        c->revAcc = nullptr;
        c->crossStale = true;
    }
    c->dp.hasGhosts = (c->hasGhosts ? 1u : 0u) | (c->pairsOnce ? 2u : 0u);
    // detection scratch
    if (int rc = sphere_scratch_for_counts(c, nS))
        return rc;
    if (int rc = grow_incidence_arena(c, std::max<size_t>(8 * nS, 4096)))
        return rc;
    c->nTri = s->nTri;  // before the contact arena: its mesh work-list buffers exist only when triangles do
    if (c->twOn && c->twTri != c->nTri)  // the wear sums of another mesh mean nothing for this one: cleared at the new size
        if (int rc = tri_wear_clear(c))
            return rc;
    if (int rc = grow_contact_arena(c, std::max<size_t>(6 * nS, 4096)))
        return rc;
    // triangles
    if (s->nTri) {
        if (!s->ownerMesh || !s->triNode1 || !s->triNode2 || !s->triNode3)
            return fail(c, DEME_ERR_INVALID, "nTri > 0 but triangle arrays are missing");
        std::vector<TriRec> ht(s->nTri);
        for (uint32_t t = 0; t < s->nTri; t++) {
            for (int k = 0; k < 3; k++) {
                ht[t].n1[k] = s->triNode1[3 * t + k];
                ht[t].n2[k] = s->triNode2[3 * t + k];
                ht[t].n3[k] = s->triNode3[3 * t + k];
            }
            ht[t].owner = s->ownerMesh[t];
            ht[t].mat = s->triMaterialOffset ? s->triMaterialOffset[t] : 0;
            ht[t].pad = 0;
            if (ht[t].owner >= s->nOwners)
                return fail(c, DEME_ERR_INVALID, "triangle %u refers to owner %u of %u", t, ht[t].owner, s->nOwners);
        }
        if (int rc = upload(c, c->tris, ht.data(), ht.size()))
            return rc;
        const size_t nT = s->nTri;
        if (ensure(c, c->triWorld, nT * sizeof(TriWorld)) || ensure(c, c->triLo, nT * 16) || ensure(c, c->triHi, nT * 16) ||
            ensure(c, c->triCounts, (nT + 1) * 4) || ensure(c, c->triOffsets, (nT + 1) * 4))
            return c->lastStatus;
        size_t need = 0;
        HIPCK(rocprim::exclusive_scan(nullptr, need, c->triCounts.as<uint32_t>(), c->triOffsets.as<uint32_t>(), 0u, nT + 1,
                                      rocprim::plus<uint32_t>(), c->stream));
        if (int rc = ensure(c, c->scanTmp, need))
            return rc;
        HIPCK(hipStreamSynchronize(c->stream));
    }
    if (!c->hPersist.empty()) {  // persistent marks survive a re-upload (UpdateClumps appends) as long as their ids still exist
        c->hPersist.erase(std::remove_if(c->hPersist.begin(), c->hPersist.end(),
                                         [&](uint64_t k) {
                                             const uint32_t cls = key_class(k);
                                             const uint32_t nB = cls == DEME_KEY_CLASS_SS ? s->nSpheres : cls == DEME_KEY_CLASS_SM ? s->nTri : s->nAnal;
                                             return key_a(k) >= s->nSpheres || key_b(k) >= nB;
                                         }),
                          c->hPersist.end());
        for (auto& k : c->hPersist)
            k = order_key_in(c, k);
        std::sort(c->hPersist.begin(), c->hPersist.end());
        if (!c->hPersist.empty()) {
            if (int rc = ensure(c, c->persistKeys, c->hPersist.size() * 8))
                return rc;
            HIPCK(hipMemcpyAsync(c->persistKeys.p, c->hPersist.data(), c->hPersist.size() * 8, hipMemcpyHostToDevice, c->stream));
        }
    }
    if (int rc = order_upload_maps(c))
        return rc;
    c->haveScene = true;
    c->haveList = false;
    c->mapFresh = false;
    c->nContacts = c->nPrev = c->nWcStored = 0;
    c->listSerial++;
    c->stepsSinceCD = 0;
    refresh_dev_params(c);
    HIPCK(hipStreamSynchronize(c->stream));  // host staging vectors die here
    return DEME_OK;
}

// which kinds of column a call names (deme_owner_cols.h)
#define DEME_COL(abi, T, Rec, f) || st->abi
static inline bool owner_state_wants_pose(const DemeOwnerState* st) { return false DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL); }
static inline bool owner_state_wants_acc(const DemeOwnerState* st) { return false DEME_OWNER_COLS(DEME_COL_NONE, DEME_COL, DEME_COL_NONE); }
#undef DEME_COL

static int owner_state_io(deme_ctx* c, const DemeOwnerState* st, int dir) {
    if (int rc = check_ready(c))
        return rc;
    if (!st)
        return DEME_ERR_INVALID;
    const size_t n = c->nOwners;
    // stage: one device buffer holding every SoA column back to back
    struct Col {
        void* host;
        size_t elem;
        void** dev;
    };
    OwnerSoA soa{};
#define DEME_COL(abi, T, Rec, f) {st->abi, sizeof(T), (void**)&soa.abi},
    Col cols[] = {DEME_OWNER_COLS(DEME_COL, DEME_COL, DEME_COL)};
#undef DEME_COL
    size_t total = 0;
    for (auto& cl : cols)
        if (cl.host)
            total += ((n * cl.elem + 15) / 16) * 16;
    if (int rc = ensure(c, c->stage, std::max<size_t>(total, 16)))
        return rc;
    size_t off = 0;
    for (auto& cl : cols) {
        if (!cl.host)
            continue;
        *cl.dev = (char*)c->stage.p + off;
        if (dir == 0)
            HIPCK(hipMemcpyAsync(*cl.dev, cl.host, n * cl.elem, hipMemcpyHostToDevice, c->stream));
        off += ((n * cl.elem + 15) / 16) * 16;
    }
    // downloads see a/alpha of EVERY owner (fixed and heavy ones are only reduced on demand)
    if (dir == 1 && c->conValid && c->haveList)
        launch_full_reduction(c);
    else if (dir == 1 && c->fusedPrevValid && c->haveList && owner_state_wants_acc(st))
        if (int rc = launch_fused_step(c, true))  // the last step was a fused one: replay its force evaluation on the buffers of its start
            return rc;
    if (dir == 0 && owner_state_wants_acc(st))
        c->conValid = false;  // the caller now owns a/alpha
    AccRec* accView = c->acc.as<AccRec>();
    if (n)
        hipLaunchKernelGGL(k_pack_owners, dim3(grid_for(n)), dim3(256), 0, c->stream, (uint32_t)n,
                           c->owners.as<OwnerRec>(), accView, soa, dir, c->dp.o2e);
    if (dir == 1) {
        off = 0;
        for (auto& cl : cols) {
            if (!cl.host)
                continue;
            HIPCK(hipMemcpyAsync(cl.host, (char*)c->stage.p + off, n * cl.elem, hipMemcpyDeviceToHost, c->stream));
            off += ((n * cl.elem + 15) / 16) * 16;
        }
    }
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

// what a write of these columns into the owner records does to the context's flags: deme_upload_owner_state (all owners) and
// deme_scatter_owner_state (a few) both call it before they write
static void owner_state_written(deme_ctx* c, const DemeOwnerState* st) {
    if (st->familyID)
        c->prescDirty = true;  // owners may have changed family
    c->fusedPrevValid = false;
    if (owner_state_wants_pose(st))
        c->listStale = true;  // pose, velocity (it sizes the margins) or family (masks) changed under the K-step list
}

int deme_upload_owner_state(deme_ctx* c, const DemeOwnerState* st) {
    if (c && st)
        owner_state_written(c, st);
    else if (c)
        c->fusedPrevValid = false;
    return owner_state_io(c, st, 0);
}
int deme_download_owner_state(deme_ctx* c, DemeOwnerState* st) { return owner_state_io(c, st, 1); }

int deme_update_tri_nodes(deme_ctx* c, const float* n1, const float* n2, const float* n3) {
    if (int rc = check_ready(c))
        return rc;
    if (!c->nTri || !n1 || !n2 || !n3)
        return fail(c, DEME_ERR_INVALID, "no triangles loaded or null node arrays");
    const size_t bytes = (size_t)c->nTri * 12;
    if (int rc = ensure(c, c->stage, bytes * 3))
        return rc;
    float* d = c->stage.as<float>();
    HIPCK(hipMemcpyAsync(d, n1, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d + 3 * (size_t)c->nTri, n2, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(d + 6 * (size_t)c->nTri, n3, bytes, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pack_tris, dim3(grid_for(c->nTri)), dim3(256), 0, c->stream, c->nTri, c->tris.as<TriRec>(), d,
                       d + 3 * (size_t)c->nTri, d + 6 * (size_t)c->nTri);
    HIPCK(hipStreamSynchronize(c->stream));
    c->listStale = true;  // the facets moved under the K-step list
    return DEME_OK;
}

int deme_compute_margins(deme_ctx* c, uint32_t drift) {
    if (int rc = check_ready(c))
        return rc;
    return do_margins(c, drift);
}

int deme_set_margins(deme_ctx* c, const float* m) {
    if (int rc = check_ready(c))
        return rc;
    if (!m)
        return DEME_ERR_INVALID;
    if (int rc = ensure(c, c->stage, std::max<size_t>(c->nOwners, 4) * 4))
        return rc;
    HIPCK(hipMemcpyAsync(c->stage.p, m, (size_t)c->nOwners * 4, hipMemcpyHostToDevice, c->stream));
    if (c->nOwners)  // (a launch of no workgroups is an error, and one that stays in the runtime's state until the next call that looks
                     // at it -- a sort of another context -- reports it)
    hipLaunchKernelGGL(k_set_margins, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->nOwners,
                       c->owners.as<OwnerRec>(), c->stage.as<float>(), c->dp.o2e);
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_detect_contacts(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    return do_detect(c);
}

int deme_migrate_history(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    return do_migrate(c);
}

int deme_calc_forces(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    if (!c->haveList || c->seeded)
        return fail(c, DEME_ERR_INVALID, "no contact list yet: call deme_detect_contacts first");
    if (int rc = launch_forces(c))
        return rc;
    launch_full_reduction(c);  // stand-alone call: a/alpha of every owner (prepareAccArrays + forceToAcc)
    return DEME_OK;
}

static int launch_family_rules(deme_ctx* c, const AccRec* accp);

int deme_integrate(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    if (c->rulesFn)  // routineChecks(): family changes sit between the force evaluation and the integration (dT.cpp:2437-2443)
        if (int rc = launch_family_rules(c, c->acc.as<AccRec>()))  // the staged path always has a/alpha stored
            return rc;
    if (int rc = launch_integrate(c, AccFrom::Stored))
        return rc;
    advance_clock(c);
    return DEME_OK;
}

static int step_tail(deme_ctx* c);
static bool detection_due(deme_ctx* c);

// ---- adaptive controllers (include/deme_hip.h: DemeAdaptive) ----------------------------------------------------------
static void apply_bin_size(deme_ctx* c, double s) {
    DemeParams& h = c->hp;
    h.binSize = s;
    // hostCalcBinNum (DEM/HostSideHelpers.hpp) as SceneBuilder._calc_bin_num / DEMSolver::Initialize use it
    h.nbX = (uint32_t)(h.voxelSize * (double)(1ull << h.nvXp2) / s) + 1;
    h.nbY = (uint32_t)(h.voxelSize * (double)(1ull << h.nvYp2) / s) + 1;
    h.nbZ = (uint32_t)(h.voxelSize * (double)(1ull << h.nvZp2) / s) + 1;
    refresh_dev_params(c);
}

// the detection just timed took `ms` on the device: DEMKinematicThread::calibrateParams (DEM/kT.cpp:43-98)
static void adapt_bin_size(deme_ctx* c, double ms) {
    const DemeAdaptive& a = c->ad;
    c->binAccMs += ms;
    if (++c->binObs < std::max(1u, a.binObserveSteps))
        return;
    const double cur = c->binAccMs / (double)c->binObs, prev = c->binPrevMs;
    c->binAccMs = 0, c->binObs = 0, c->binPrevMs = cur;
    if (prev < 0)
        return;  // first window: nothing to compare with yet
    int dir = (c->binRate > 0.f) - (c->binRate < 0.f);
    if (dir == 0) {  // the reference draws a random direction here; alternate instead (reproducible runs)
        dir = c->binFlip;
        c->binFlip = -c->binFlip;
    }
    float upd = ((cur < prev) ? dir : -dir) * a.binAcc * a.binMaxRate;
    if ((double)c->maxInBin > (double)a.binUpperSafety * (double)c->dp.errOutBinSphNum)
        upd = -1.f * a.binAcc * a.binMaxRate;  // bins too full: the size must start to decrease
    const double nBins = (double)c->hp.nbX * (double)c->hp.nbY * (double)c->hp.nbZ;
    if (nBins > (double)a.binLowerSafety * 4294967295.0)
        upd = 1.f * a.binAcc * a.binMaxRate;  // too many bins for the 32-bit bin id: the size must start to increase
    c->binRate = std::min(a.binMaxRate, std::max(-a.binMaxRate, c->binRate + upd));
    double s = c->hp.binSize;
    if (c->binRate > 0.f)
        s *= 1.0 + (double)c->binRate;
    else
        s /= 1.0 - (double)c->binRate;
    const double nb = (c->hp.voxelSize * (double)(1ull << c->hp.nvXp2) / s + 1) * (c->hp.voxelSize * (double)(1ull << c->hp.nvYp2) / s + 1) *
                      (c->hp.voxelSize * (double)(1ull << c->hp.nvZp2) / s + 1);
    if (nb >= 4294967295.0)
        return;  // would overflow the bin id: keep the size
    apply_bin_size(c, s);
    c->nBinChanges++;
}

// a window of steps ending at a detection took `ms` per step: hill climb on K = cdUpdateFreq
static void adapt_update_freq(deme_ctx* c, double msPerStep) {
    const DemeAdaptive& a = c->ad;
    const double prev = c->freqPrevMs;
    c->freqPrevMs = msPerStep;
    if (prev >= 0 && msPerStep >= prev)
        c->freqDir = -c->freqDir;  // no improvement: turn round
    const uint32_t K = std::max(1u, c->hp.cdUpdateFreq), hi = std::max(1u, a.maxUpdateFreq);
    const uint32_t stepK = std::max(1u, K / 8);
    const uint32_t nK = c->freqDir > 0 ? std::min(hi, K + stepK) : (K > stepK ? K - stepK : 1u);
    if (nK != K) {
        c->hp.cdUpdateFreq = nK;
        refresh_dev_params(c);
        c->nFreqChanges++;
    }
}

static int ensure_adaptive_events(deme_ctx* c) {
    if (c->evDet0)
        return DEME_OK;
    HIPCK(hipEventCreate(&c->evDet0));
    HIPCK(hipEventCreate(&c->evDet1));
    HIPCK(hipEventCreate(&c->evWin0));
    HIPCK(hipEventCreate(&c->evWin1));
    return DEME_OK;
}

// margins + detection + history migration of a step whose list is due, with the controllers' timing around it
static int order_renew(deme_ctx* c);
static int detection_phase(deme_ctx* c) {
    if (c->orderRenewDue && !c->inGroupStep)  // (asynchronous cycles begin and end inside deme_step: none is in flight here)
        if (int rc = order_renew(c))
            return rc;
    const bool adaptive = c->ad.autoBinSize || c->ad.autoUpdateFreq;
    if (adaptive) {
        if (int rc = ensure_adaptive_events(c))
            return rc;
        if (c->ad.autoUpdateFreq && c->hp.cdUpdateFreq > 0) {
            if (c->winOpen && ++c->freqObs >= std::max(1u, c->ad.freqObserveDetections)) {
                HIPCK(hipEventRecord(c->evWin1, c->stream));
                HIPCK(hipEventSynchronize(c->evWin1));
                float ms = 0.f;
                HIPCK(hipEventElapsedTime(&ms, c->evWin0, c->evWin1));
                const uint64_t n = c->nSteps - c->winStartStep;
                if (n)
                    adapt_update_freq(c, (double)ms / (double)n);
                c->winOpen = false;
            }
            if (!c->winOpen) {  // a window starts at a detection and includes it
                HIPCK(hipEventRecord(c->evWin0, c->stream));
                c->winStartStep = c->nSteps, c->freqObs = 0, c->winOpen = true;
            }
        }
        if (c->ad.autoBinSize)
            HIPCK(hipEventRecord(c->evDet0, c->stream));
    }
    if (int rc = do_margins(c, c->hp.cdUpdateFreq))
        return rc;
    if (int rc = do_detect(c))
        return rc;
    if (adaptive && c->ad.autoBinSize) {
        HIPCK(hipEventRecord(c->evDet1, c->stream));
        HIPCK(hipEventSynchronize(c->evDet1));  // (do_detect ended on a synchronisation: nothing is queued behind)
        float ms = 0.f;
        HIPCK(hipEventElapsedTime(&ms, c->evDet0, c->evDet1));
        adapt_bin_size(c, (double)ms);
    }
    if (int rc = do_migrate(c))
        return rc;
    c->stepsSinceCD = 0;
    c->listStale = false;
    return DEME_OK;
}

int deme_set_adaptive(deme_ctx* c, const DemeAdaptive* a) {
    if (!c || !a)
        return DEME_ERR_INVALID;
    if (a->autoBinSize && (!(a->binMaxRate >= 0.f) || !(a->binAcc > 0.f)))
        return fail(c, DEME_ERR_INVALID, "deme_set_adaptive: binMaxRate must be >= 0 and binAcc > 0");
    c->ad = *a;
    c->binAccMs = 0, c->binPrevMs = -1, c->freqPrevMs = -1, c->binRate = 0.f, c->binObs = 0, c->freqObs = 0, c->winOpen = false;
    return DEME_OK;
}

int deme_get_adaptive_state(deme_ctx* c, double* binSize, uint32_t* cdUpdateFreq, uint32_t* nBinChanges, uint32_t* nFreqChanges) {
    if (!c)
        return DEME_ERR_INVALID;
    if (binSize)
        *binSize = c->hp.binSize;
    if (cdUpdateFreq)
        *cdUpdateFreq = c->hp.cdUpdateFreq;
    if (nBinChanges)
        *nBinChanges = c->nBinChanges;
    if (nFreqChanges)
        *nFreqChanges = c->nFreqChanges;
    return DEME_OK;
}

// ---- asynchronous detection ---------------------------------------------------------------------------------------------------
// K - D steps after a list was swapped in (D = asyncLead), the owners are copied, the next D steps are enqueued on the main stream
// with the CURRENT list, and part 1 of the detection runs beside them on its own stream from the copy, with margins for the K + D
// steps that pass between the copy and the end of the new list's service.  When the D steps are enqueued the main stream waits for
// part 1, builds the gather lists (part 2), migrates the history, and carries on with the new list.  The host blocks in part 1's
// two sizing read-backs while the GPU works through the D steps: no second host thread is needed.  Contacts are never missed (the
// margins cover the whole span); the new list holds a few more near-pairs than a lock-step detection would, whose contributions are
// zero, so a trajectory in the exact arithmetic mode is the lock-step one.
static bool async_detection_can_start(deme_ctx* c, uint32_t stepsLeftInCall) {
    const uint32_t K = c->hp.cdUpdateFreq, D = c->asyncLead;
    if (!D || K <= D || stepsLeftInCall < D)
        return false;
    // (a mesh, ghosts and marked contacts are fine: part 1 reads the owner snapshot, static scene data and the marked set, and
    // writes detection scratch only; whatever changes them between detections marks the list stale, and a stale list is rebuilt
    // in lock-step.  Replicated free owners and the adaptive controllers -- which time a detection on the main stream -- stay
    // with the lock-step detection.)
    if (!c->haveList || c->seeded || c->listStale || c->mapFresh || !c->hShared.empty())
        return false;
    if (c->ad.autoBinSize || c->ad.autoUpdateFreq)
        return false;
    return c->stepsSinceCD == K - D;
}
static int async_stream(deme_ctx* c) {  // the detection stream and its two events, made once
    if (c->detStream)
        return DEME_OK;
    HIPCK(hipStreamCreateWithFlags(&c->detStream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&c->evSnap, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->evP1, hipEventDisableTiming));
    return DEME_OK;
}
// the three phases of one asynchronous detection: the owner snapshot (on the main stream, between two integrations), part 1 beside
// the next D steps, the swap
static int async_snapshot(deme_ctx* c) {
    if (int rc = async_stream(c))
        return rc;
    if (int rc = ensure(c, c->ownersSnap, (size_t)c->nOwners * sizeof(OwnerRec)))
        return rc;
    HIPCK(hipMemcpyAsync(c->ownersSnap.p, c->owners.p, (size_t)c->nOwners * sizeof(OwnerRec), hipMemcpyDeviceToDevice, c->stream));
    HIPCK(hipEventRecord(c->evSnap, c->stream));
    c->snapPending = false;
    return DEME_OK;
}
static int async_part1(deme_ctx* c, uint64_t* nC) {
    const uint32_t K = c->hp.cdUpdateFreq, D = c->asyncLead;
    HIPCK(hipStreamWaitEvent(c->detStream, c->evSnap, 0));
    ScopedTimer tm(c, "detect_async_part1", true, c->detStream);
    if (int rc = launch_margins(c, c->detStream, c->ownersSnap.as<OwnerRec>(), K + D))
        return rc;
    if (int rc = detect_part1(c, c->detStream, c->ownersSnap.as<OwnerRec>(), true, nC))
        return rc;
    HIPCK(hipEventRecord(c->evP1, c->detStream));
    return DEME_OK;
}
// the list an asynchronous detection builds, at the sizes of the arenas and the scene; nothing in flight reads it
static int async_size_next(deme_ctx* c) {
    ContactList& N = c->list[c->cur ^ 1];
    if (int rc = size_list_per_contact(c, N, c->cntCap, c->hasGhosts, c->nTri))
        return rc;
    return size_list_per_owner(c, N, c->nOwners);
}
// streams, events and buffers of the asynchronous detection, made when it is switched on (a first cycle that allocates a
// gigabyte of list structures inside a short timed run costs more than the detection it hides)
static int async_prepare(deme_ctx* c) {
    if (int rc = async_stream(c))
        return rc;
    if (!c->haveParams || !c->haveScene)
        return DEME_OK;
    if (int rc = ensure(c, c->ownersSnap, (size_t)c->nOwners * sizeof(OwnerRec)))
        return rc;
    if (int rc = ensure(c, c->keysMid, (size_t)c->cntCap * 8))
        return rc;
    return async_size_next(c);
}
// Part 2 beside the steps: every step that reads the current list has been enqueued, the other list is built on the detection
// stream from the snapshot, and the index flips once that has succeeded.  A failure leaves the current list -- buffers and
// description alike -- as the steps know it.
static int async_part2(deme_ctx* c, uint64_t nC) {
    ContactList& N = c->list[c->cur ^ 1];
    if (int rc = async_size_next(c))
        return rc;
    {
        ScopedTimer tm(c, "detect_async_part2", true, c->detStream);
        HIPCK(hipMemsetAsync(N.heavy.p, 0, N.heavy.bytes, c->detStream));
        HIPCK(hipMemsetAsync(N.fixedFlag.p, 0, N.fixedFlag.bytes, c->detStream));
        if (int rc = detect_part2(c, N, c->ownersSnap.as<OwnerRec>(), c->detStream, nC))
            return rc;
    }
    c->cur ^= 1;
    HIPCK(hipEventRecord(c->evP1, c->detStream));
    HIPCK(hipStreamWaitEvent(c->stream, c->evP1, 0));
    if (int rc = do_migrate(c))  // the history follows its contacts into the new order: with the wildcards the last step left
        return rc;
    c->stepsSinceCD = 0;
    c->listStale = false;
    c->nAsyncDetections++;
    return DEME_OK;
}
static int async_detection_cycle(deme_ctx* c) {
    const uint32_t D = c->asyncLead;
    // the copy is ordered on the main stream: after the step just integrated, before the next one
    if (int rc = async_snapshot(c))
        return rc;
    for (uint32_t d = 0; d < D; d++) {  // D steps with the current list (its margins were sized for them)
        if (int rc = launch_forces(c))
            return rc;
        if (int rc = step_tail(c))
            return rc;
    }
    uint64_t nC = 0;
    if (int rc = async_part1(c, &nC))
        return rc;
    return async_part2(c, nC);
}

int deme_set_async_detection(deme_ctx* c, uint32_t leadSteps) {
    if (!c)
        return DEME_ERR_INVALID;
    c->asyncLead = leadSteps;
    if (leadSteps) {
        hipSetDevice(c->device);
        return async_prepare(c);
    }
    return DEME_OK;
}

int deme_step(deme_ctx* c, uint32_t nsteps) {
    if (int rc = check_ready(c))
        return rc;
    if (!c->hShared.empty())
        return fail(c, DEME_ERR_INVALID, "this slab holds replicated free owners: step it through deme_halo_group_step, which adds their accelerations up across the slabs");
    for (uint32_t i = 0; i < nsteps; i++) {
        if (c->orderRenewDue && !c->inGroupStep && async_detection_can_start(c, nsteps - i)) {
            // the order is to be renewed: this update is a lock-step one (the renewal is host-driven and needs the context idle)
            if (int rc = detection_phase(c))
                return rc;
        } else if (async_detection_can_start(c, nsteps - i)) {
            if (int rc = async_detection_cycle(c))
                return rc;
            i += c->asyncLead - 1;
            continue;
        }
        if (detection_due(c))
            if (int rc = detection_phase(c))
                return rc;
        if (fused_ready(c)) {  // the whole step in one launch: closed tiles integrate their own owners (deme_tile_step.h)
            if (int rc = launch_fused_step(c, false))
                return rc;
            continue;
        }
        c->fusedPrevValid = false;
        if (int rc = launch_forces(c))
            return rc;
        if (int rc = step_tail(c))
            return rc;
    }
    return DEME_OK;
}

static int launch_family_rules(deme_ctx* c, const AccRec* accp) {
    OwnerRec* ow = c->owners.as<OwnerRec>();
    uint32_t n = c->nOwners;
    float t = (float)c->timeElapsed;
    void* args[] = {&c->dp, &ow, &accp, &n, &t};
    HIPCK(hipModuleLaunchKernel(c->rulesFn, grid_for(n), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
    return DEME_OK;
}

// rules + integration + bookkeeping of one step (after the force evaluation), in two halves: everything that produces the
// separately reduced a / alpha (heavy and replicated owners), then the integration.  A slab group adds the replicated owners'
// sums up across slabs between the two (deme_halo_group_step).
static int step_tail_pre(deme_ctx* c) {
    ContactList& L = c->list[c->cur];
    bool fused = true;
    if (c->rulesFn) {  // routineChecks(): applyFamilyChanges between forces and integration (dT.cpp:2437-2443)
        const AccRec* accp = nullptr;
        if (c->rulesNeedAcc) {
            launch_full_reduction(c);
            accp = c->acc.as<AccRec>();
            fused = false;
        }
        if (int rc = launch_family_rules(c, accp))
            return rc;
    }
    c->tailFused = fused;
    if (fused)
        launch_reduce_heavy(c, true);
    if (L.heavyOverflow)
        return c->lastStatus;
    return DEME_OK;
}
// Owners::NotWaiting (slab group, one evaluation per cross-cut contact): this half of the step leaves out the owners that wait for a
// reverse share and returns before the step's bookkeeping -- step_tail_later finishes it when the share has arrived
static int step_tail_post(deme_ctx* c, Owners who = Owners::All) {
    if (int rc = launch_integrate(c, c->tailFused ? AccFrom::Contributions : AccFrom::Stored, who))
        return rc;
    return who == Owners::NotWaiting ? DEME_OK : finish_step(c);
}
static int step_tail(deme_ctx* c) {
    if (int rc = step_tail_pre(c))
        return rc;
    return step_tail_post(c);
}
static int step_tail_later(deme_ctx* c, const uint32_t* ids, uint32_t n) {
    if (int rc = launch_integrate_later(c, ids, n))
        return rc;
    return finish_step(c);
}

static bool detection_due(deme_ctx* c) {
    const uint32_t K = c->hp.cdUpdateFreq;
    return !c->haveList || c->seeded || c->listStale || K == 0 || c->stepsSinceCD >= K;
}

static int ensure_halo_stream(deme_ctx* c) {
    if (c->haloStream)
        return DEME_OK;
    HIPCK(hipStreamCreateWithFlags(&c->haloStream, hipStreamNonBlocking));
    HIPCK(hipEventCreateWithFlags(&c->evStepDone, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&c->evHaloDone, hipEventDisableTiming));
    HIPCK(hipEventRecord(c->evStepDone, c->stream));
    return DEME_OK;
}

int deme_halo_stream(deme_ctx* c, void** stream) {
    if (!c || !stream)
        return DEME_ERR_INVALID;
    if (int rc = ensure_halo_stream(c))
        return rc;
    *stream = (void*)c->haloStream;
    return DEME_OK;
}

int deme_halo_pack_async(deme_ctx* c, const uint32_t* d_ids, uint32_t n, void* d_buf) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = ensure_halo_stream(c))
        return rc;
    HIPCK(hipStreamWaitEvent(c->haloStream, c->evStepDone, 0));  // the owners' state of the step just integrated
    if (n)
        hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n)), dim3(256), 0, c->haloStream, n, d_ids, c->owners.as<OwnerRec>(),
                           (GhostRec*)d_buf);
    return DEME_OK;
}

int deme_halo_unpack_async(deme_ctx* c, const uint32_t* d_ids, uint32_t n, const void* d_buf) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = ensure_halo_stream(c))
        return rc;
    if (n)
        hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(n)), dim3(256), 0, c->haloStream, n, d_ids, c->owners.as<OwnerRec>(),
                           (const GhostRec*)d_buf);
    HIPCK(hipEventRecord(c->evHaloDone, c->haloStream));
    return DEME_OK;
}

int deme_halo_sync(deme_ctx* c) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    if (c->haloStream)
        HIPCK(hipStreamSynchronize(c->haloStream));
    return DEME_OK;
}

int deme_step_overlap_begin(deme_ctx* c, int* detectionDue) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = ensure_halo_stream(c))
        return rc;
    c->overlapDetect = detection_due(c) || !c->hasGhosts;
    if (detectionDue)
        *detectionDue = c->overlapDetect ? 1 : 0;
    if (c->overlapDetect)
        return DEME_OK;  // a detection reads the ghosts' new positions: nothing can start before they are in place
    return launch_forces(c, 0);
}

// second half of an overlapped step up to (not including) the tail: the detection if one is due, the remaining force pass
static int overlap_forces(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = ensure_halo_stream(c))
        return rc;
    HIPCK(hipStreamWaitEvent(c->stream, c->evHaloDone, 0));
    if (c->snapPending)  // an asynchronous detection starts from this moment: own clumps and ghosts both hold the state of the step just integrated
        if (int rc = async_snapshot(c))
            return rc;
    if (c->overlapDetect) {
        c->overlapDetect = false;
        if (detection_due(c))
            if (int rc = detection_phase(c))
                return rc;
        return launch_forces(c);
    }
    return launch_forces(c, 1);
}

int deme_step_overlap_end(deme_ctx* c) {
    if (c && !c->hShared.empty() && !c->inGroupStep)
        return fail(c, DEME_ERR_INVALID, "this slab holds replicated free owners: step it through deme_halo_group_step, which adds their accelerations up across the slabs");
    if (int rc = overlap_forces(c))
        return rc;
    return step_tail(c);
}

// ================================================================================================
// Slab halo exchange driven from the library: RCCL send / recv of the packed ghost records between face neighbours, on its own
// stream, overlapped with the interior force evaluation (north_star; SURVEY 8e "ncclGroupStart; ncclSend/ncclRecv ...").
// RCCL is bound at run time (dlopen): a process that has PyTorch loaded shares PyTorch's copy, and libdeme_hip.so has no
// link-time dependency on it.
// ================================================================================================
namespace {
typedef struct ncclComm* ncclComm_t;
typedef struct {
    char internal[128];
} ncclUniqueId_t;
struct RcclApi {
    void* lib = nullptr;
    int (*GetUniqueId)(ncclUniqueId_t*) = nullptr;
    int (*CommInitRank)(ncclComm_t*, int, ncclUniqueId_t, int) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    int (*CommCount)(ncclComm_t, int*) = nullptr;
    std::string err;
};
RcclApi* rccl_api() {
    static RcclApi api;
    if (api.lib || !api.err.empty())
        return &api;
    // PyTorch's copy first if the process already holds it, then the ROCm installation's
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        if (h)
            break;
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!h) {
        api.err = std::string("RCCL could not be loaded: ") + (dlerror() ? dlerror() : "librccl.so not found");
        return &api;
    }
    bool ok = true;
    auto sym = [&](const char* n) {
        void* p = dlsym(h, n);
        ok = ok && p;
        return p;
    };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
    if (!ok) {
        api.err = "librccl.so lacks one of the entry points (send / recv / all-reduce)";
        return &api;
    }
    api.lib = h;
    return &api;
}
constexpr int kNcclUint8 = 1;  // ncclUint8 (rccl.h: ncclInt8 = 0, ncclUint8 = 1)
constexpr int kNcclFloat32 = 7, kNcclSum = 0;  // rccl.h: ncclFloat32 = 7; ncclSum = 0

struct HaloSide {
    int peerRank = -1;          // rank that holds the neighbouring slab, -1: none (end of the chain)
    deme_ctx* peerLocal = nullptr;  // the neighbour's context when this process holds it too
    void *sendIds = nullptr, *recvIds = nullptr, *sendBuf = nullptr, *recvBuf = nullptr;
    uint32_t nSend = 0, nRecv = 0;
    // one evaluation per cross-cut contact: a / alpha of the sums this slab evaluated for its RIGHT ghosts travel to their owner
    // (right side: nRecv x 32 bytes out), those the left neighbour evaluated for this slab's clumps come back (left side: nSend x
    // 32 bytes in) -- the lists of the forward exchange, read the other way round
    void* revBuf = nullptr;
    uint32_t revCap = 0;
};
struct MigBuf {  // one direction of a migration exchange: clumps, their spheres, history rows (device buffers, counts on the host)
    void *clumps = nullptr, *spheres = nullptr, *rowH = nullptr, *rowW = nullptr, *counts = nullptr;
    void *owc = nullptr, *swc = nullptr;  // user wildcard arrays of the clumps / spheres: [clump][k], [sphere][k] floats
    uint32_t nC = 0, nS = 0, nR = 0;
    bool borrowed = false;  // the buffers belong to a neighbour slab of this process
};
struct MigPool {  // the scratch of one slab's migrations: one device block, kept between calls (three dozen hipMalloc / hipFree
                  // pairs per call cost more than the kernels of a migration)
    void* base = nullptr;
    size_t cap = 0, lastNeed = 0;
};
struct SlabGeom {  // what deme_halo_group_migrate needs to know about a slab (deme_halo_group_set_slab)
    bool set = false;
    void *ownerGid = nullptr, *sphereGid = nullptr;
    size_t gidCapO = 0, gidCapS = 0;
    double xLo = 0, xHi = 0, halo = 0;
    uint32_t nOwn = 0, nGL = 0, nGR = 0, flipMask = 7u;
};
struct HaloSlab {
    deme_ctx* ctx = nullptr;
    SlabGeom geo;
    HaloSide side[2];  // 0 left, 1 right
    hipEvent_t evPacked = nullptr;
    hipEvent_t evAcc = nullptr;  // this slab's share of the replicated owners' a / alpha is in its buffer
    hipEvent_t evRev = nullptr;  // the sums of this slab's right ghosts are packed
    uint32_t nOwnersAtAttach = 0;
    MigPool pool;
};
}  // namespace

struct deme_halo_group {
    RcclApi* api = nullptr;
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1, device = 0;
    hipStream_t xstream = nullptr;  // the exchange runs here: after every slab's pack, before every slab's unpack
    hipEvent_t evExchanged = nullptr;
    hipEvent_t evRevDone = nullptr;
    bool pairsOnce = false;  // deme_halo_group_set_cross_contacts: one evaluation per cross-cut contact, reactions sent back
    uint64_t nRevExchanges = 0;
    std::vector<HaloSlab> slabs;
    int axis = 0;                    // the axis the slabs were cut along (deme_halo_group_set_axis / _build): what "left" and "right" mean
    uint32_t firstSlab = 0;          // number of this rank's first slab in the whole chain (deme_halo_group_build)
    std::vector<deme_ctx*> ownedCtx; // contexts deme_halo_group_build created: destroyed with the group
    uint32_t nOwnersGlobal = 0, nClumpsGlobal = 0;
    uint32_t nShared = 0;            // replicated free owners (the same on every slab): a / alpha summed across slabs every step
    void* sharedSum = nullptr;       // nShared x AccRec
    void* agreeBuf = nullptr;        // 16 bytes: the error flag the ranks add up before a collective phase (mig_agree)
    bool anyPersist = false;         // (during a migration) some slab of some rank holds persistent marks: the rows carry them
    hipEvent_t evReduced = nullptr;
    std::string err;
    uint64_t nExchanges = 0, nReductions = 0, bytesPerStep = 0;
    double hostUs[4] = {0, 0, 0, 0};  // host time spent enqueuing: interior pass, pack, RCCL group, unpack + boundary pass + integration
};

namespace {
int gfail(deme_halo_group* g, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (g)
        g->err = buf;
    return code;
}
#define GHIP(call)                                                                                             \
    do {                                                                                                       \
        hipError_t _e = (call);                                                                                \
        if (_e != hipSuccess)                                                                                  \
            return gfail(g, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define GNCCL(call)                                                                                             \
    do {                                                                                                        \
        int _r = (call);                                                                                        \
        if (_r != 0)                                                                                            \
            return gfail(g, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, g->api->GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)
}  // namespace

int deme_halo_unique_id(unsigned char* id128) {
    RcclApi* api = rccl_api();
    if (!api->lib || !id128)
        return DEME_ERR_HIP;
    ncclUniqueId_t id;
    if (api->GetUniqueId(&id) != 0)
        return DEME_ERR_HIP;
    memcpy(id128, id.internal, 128);
    return DEME_OK;
}

int deme_halo_group_create(const unsigned char* id128, int rank, int world, int device, deme_halo_group** out) {
    if (!out || world < 1 || rank < 0 || rank >= world)
        return DEME_ERR_INVALID;
    *out = nullptr;
    deme_halo_group* g = new deme_halo_group();
    g->api = rccl_api();
    g->rank = rank, g->world = world, g->device = device;
    *out = g;  // returned even on failure so that deme_halo_group_last_error can report
    if (!g->api->lib)
        return gfail(g, DEME_ERR_HIP, "%s", g->api->err.c_str());
    GHIP(hipSetDevice(device));
    ncclUniqueId_t id;
    if (id128)
        memcpy(id.internal, id128, 128);
    else if (world == 1)
        GNCCL(g->api->GetUniqueId(&id));  // a one-rank communicator: sends to self serve the slabs one process holds
    else
        return gfail(g, DEME_ERR_INVALID, "a communicator of %d ranks needs the unique id rank 0 generated", world);
    GNCCL(g->api->CommInitRank(&g->comm, world, id, rank));
    GHIP(hipStreamCreateWithFlags(&g->xstream, hipStreamNonBlocking));
    GHIP(hipEventCreateWithFlags(&g->evExchanged, hipEventDisableTiming));
    return DEME_OK;
}

void deme_halo_group_destroy(deme_halo_group* g) {
    if (!g)
        return;
    hipSetDevice(g->device);
    if (g->xstream)
        hipStreamSynchronize(g->xstream);
    for (auto& s : g->slabs) {
        if (s.ctx && s.ctx->haloStream)
            hipStreamSynchronize(s.ctx->haloStream);
        for (auto& sd : s.side)
            for (void* p : {sd.sendIds, sd.recvIds, sd.sendBuf, sd.recvBuf})
                if (p)
                    hipFree(p);
        if (s.evPacked)
            hipEventDestroy(s.evPacked);
        if (s.evAcc)
            hipEventDestroy(s.evAcc);
        if (s.evRev)
            hipEventDestroy(s.evRev);
        if (s.pool.base)
            hipFree(s.pool.base);
        for (auto& sd : s.side)
            if (sd.revBuf)
                hipFree(sd.revBuf);
        // the slab's books of global ids (deme_halo_group_set_slab / every migration allocates them anew; a decomposed run that is
        // re-planned -- UpdateClumps, ResortClumps, ReplanSlabs -- destroys and rebuilds its groups each time)
        if (s.geo.ownerGid)
            hipFree(s.geo.ownerGid);
        if (s.geo.sphereGid)
            hipFree(s.geo.sphereGid);
        s.geo.ownerGid = s.geo.sphereGid = nullptr;
    }
    if (g->evRevDone)
        hipEventDestroy(g->evRevDone);
    if (g->sharedSum)
        hipFree(g->sharedSum);
    if (g->agreeBuf)
        hipFree(g->agreeBuf);
    if (g->evReduced)
        hipEventDestroy(g->evReduced);
    if (g->comm)
        g->api->CommDestroy(g->comm);
    if (g->evExchanged)
        hipEventDestroy(g->evExchanged);
    if (g->xstream)
        hipStreamDestroy(g->xstream);
    for (deme_ctx* c : g->ownedCtx)
        deme_ctx_destroy(c);
    delete g;
}

const char* deme_halo_group_last_error(const deme_halo_group* g) { return g ? g->err.c_str() : "null halo group"; }

int deme_halo_group_attach(deme_halo_group* g, deme_ctx* c, int leftRank, deme_ctx* leftLocal, const uint32_t* sendLeft,
                           uint32_t nSendLeft, const uint32_t* recvLeft, uint32_t nRecvLeft, int rightRank, deme_ctx* rightLocal,
                           const uint32_t* sendRight, uint32_t nSendRight, const uint32_t* recvRight, uint32_t nRecvRight) {
    if (!g || !c || !g->comm)
        return DEME_ERR_INVALID;
    if (int rc = check_ready(c))
        return gfail(g, rc, "attach: %s", c->err.c_str());
    if (int rc = ensure_halo_stream(c))
        return gfail(g, rc, "attach: %s", c->err.c_str());
    HaloSlab s;
    s.ctx = c;
    GHIP(hipEventCreateWithFlags(&s.evPacked, hipEventDisableTiming));
    GHIP(hipEventCreateWithFlags(&s.evAcc, hipEventDisableTiming));
    {   // replicated free owners: the same list, in the same order, on every slab of every rank (decomp.py keeps them so)
        const uint32_t n = (uint32_t)c->hShared.size();
        if (!g->slabs.empty() && n != g->nShared)
            return gfail(g, DEME_ERR_INVALID, "attach: this slab has %u replicated free owners, the slabs before it %u", n, g->nShared);
        g->nShared = n;
        if (n) {
            if (ensure(c, c->sharedBuf, (size_t)n * sizeof(AccRec)))
                return gfail(g, c->lastStatus, "attach: %s", c->err.c_str());
            if (!g->sharedSum) {
                GHIP(hipMalloc(&g->sharedSum, (size_t)n * sizeof(AccRec)));
                GHIP(hipEventCreateWithFlags(&g->evReduced, hipEventDisableTiming));
            }
        }
    }
    const int peer[2] = {leftRank, rightRank};
    deme_ctx* local[2] = {leftLocal, rightLocal};
    const uint32_t* sIds[2] = {sendLeft, sendRight};
    const uint32_t* rIds[2] = {recvLeft, recvRight};
    const uint32_t nS[2] = {nSendLeft, nSendRight}, nR[2] = {nRecvLeft, nRecvRight};
    for (int k = 0; k < 2; k++) {
        HaloSide& sd = s.side[k];
        sd.peerRank = peer[k], sd.peerLocal = local[k], sd.nSend = nS[k], sd.nRecv = nR[k];
        if (peer[k] < 0)
            continue;
        if (peer[k] >= g->world || (peer[k] == g->rank) != (local[k] != nullptr))
            return gfail(g, DEME_ERR_INVALID, "attach: neighbour rank %d of %d; a neighbour on this rank must be given as a context", peer[k], g->world);
        for (uint32_t i = 0; i < nS[k]; i++)
            if (sIds[k][i] >= c->nOwners)
                return gfail(g, DEME_ERR_INVALID, "attach: send id %u out of range", sIds[k][i]);
        for (uint32_t i = 0; i < nR[k]; i++)
            if (rIds[k][i] >= c->nOwners)
                return gfail(g, DEME_ERR_INVALID, "attach: receive id %u out of range", rIds[k][i]);
        GHIP(hipMalloc(&sd.sendIds, std::max<size_t>(nS[k], 1) * 4));
        GHIP(hipMalloc(&sd.recvIds, std::max<size_t>(nR[k], 1) * 4));
        GHIP(hipMalloc(&sd.sendBuf, std::max<size_t>(nS[k], 1) * sizeof(GhostRec)));
        GHIP(hipMalloc(&sd.recvBuf, std::max<size_t>(nR[k], 1) * sizeof(GhostRec)));
        std::vector<uint32_t> ts, tr;
        const uint32_t *ps = sIds[k], *pr = rIds[k];
        if (c->permuted) {  // (a context with its own order holds no ghosts, so these lists are empty in practice)
            ts.assign(ps, ps + nS[k]), tr.assign(pr, pr + nR[k]);
            for (auto& v : ts)
                v = c->hE2O[v];
            for (auto& v : tr)
                v = c->hE2O[v];
            ps = ts.data(), pr = tr.data();
        }
        if (nS[k])
            GHIP(hipMemcpy(sd.sendIds, ps, (size_t)nS[k] * 4, hipMemcpyHostToDevice));
        if (nR[k])
            GHIP(hipMemcpy(sd.recvIds, pr, (size_t)nR[k] * 4, hipMemcpyHostToDevice));
        g->bytesPerStep += (uint64_t)nS[k] * sizeof(GhostRec);
    }
    s.nOwnersAtAttach = c->nOwners;
    g->slabs.push_back(s);
    return DEME_OK;
}

// one exchange of every slab's ghost records: pack on each slab's halo stream, all transfers in ONE RCCL group on the exchange
// stream, unpack on each slab's halo stream again
static inline double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static int halo_exchange(deme_halo_group* g) {
    const double t0 = now_us();
    for (auto& s : g->slabs) {
        deme_ctx* c = s.ctx;
        GHIP(hipStreamWaitEvent(c->haloStream, c->evStepDone, 0));  // the owners' state of the step just integrated
        for (auto& sd : s.side)
            if (sd.peerRank >= 0 && sd.nSend)
                hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(sd.nSend)), dim3(256), 0, c->haloStream, sd.nSend, (const uint32_t*)sd.sendIds,
                                   c->owners.as<OwnerRec>(), (GhostRec*)sd.sendBuf);
        GHIP(hipEventRecord(s.evPacked, c->haloStream));
        GHIP(hipStreamWaitEvent(g->xstream, s.evPacked, 0));
    }
    auto find = [&](deme_ctx* c) -> HaloSlab* {
        for (auto& s : g->slabs)
            if (s.ctx == c)
                return &s;
        return nullptr;
    };
    for (auto& s : g->slabs) {  // every check that can fail comes BEFORE the group opens: an RCCL group left open hangs what follows
        HaloSide& r = s.side[1];
        if (r.peerRank >= 0 && r.peerLocal) {
            HaloSlab* nb = find(r.peerLocal);
            if (!nb)
                return gfail(g, DEME_ERR_INVALID, "a local neighbour context is not attached to the group");
            HaloSide& l = nb->side[0];
            if (l.nRecv != r.nSend || l.nSend != r.nRecv)
                return gfail(g, DEME_ERR_INVALID, "ghost lists of two neighbouring slabs do not match (%u/%u vs %u/%u)", r.nSend, r.nRecv, l.nRecv, l.nSend);
        }
    }
    const double t1 = now_us();
    g->hostUs[1] += t1 - t0;
    GNCCL(g->api->GroupStart());
#define GNCCL_IN_GROUP(call)                                                                                                     \
    do {                                                                                                                         \
        int _r = (call);                                                                                                         \
        if (_r != 0) {                                                                                                           \
            g->api->GroupEnd();                                                                                                  \
            return gfail(g, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, g->api->GetErrorString(_r), __FILE__, __LINE__);        \
        }                                                                                                                        \
    } while (0)
    for (auto& s : g->slabs) {
        // the right-hand edge of every slab (each edge once).  A neighbour in this process: the two transfers go to self, and
        // sends to self meet receives from self in posting order -- so each send is posted right before the receive it feeds
        HaloSide& r = s.side[1];
        if (r.peerRank >= 0) {
            if (r.peerLocal) {
                HaloSide& l = find(r.peerLocal)->side[0];  // (checked above)
                if (r.nSend) {
                    GNCCL_IN_GROUP(g->api->Send(r.sendBuf, (size_t)r.nSend * sizeof(GhostRec), kNcclUint8, g->rank, g->comm, g->xstream));
                    GNCCL_IN_GROUP(g->api->Recv(l.recvBuf, (size_t)l.nRecv * sizeof(GhostRec), kNcclUint8, g->rank, g->comm, g->xstream));
                }
                if (l.nSend) {
                    GNCCL_IN_GROUP(g->api->Send(l.sendBuf, (size_t)l.nSend * sizeof(GhostRec), kNcclUint8, g->rank, g->comm, g->xstream));
                    GNCCL_IN_GROUP(g->api->Recv(r.recvBuf, (size_t)r.nRecv * sizeof(GhostRec), kNcclUint8, g->rank, g->comm, g->xstream));
                }
            } else {
                if (r.nSend)
                    GNCCL_IN_GROUP(g->api->Send(r.sendBuf, (size_t)r.nSend * sizeof(GhostRec), kNcclUint8, r.peerRank, g->comm, g->xstream));
                if (r.nRecv)
                    GNCCL_IN_GROUP(g->api->Recv(r.recvBuf, (size_t)r.nRecv * sizeof(GhostRec), kNcclUint8, r.peerRank, g->comm, g->xstream));
            }
        }
        HaloSide& l = s.side[0];
        if (l.peerRank >= 0 && !l.peerLocal) {  // a left neighbour on another rank (a local one was served as its right edge)
            if (l.nSend)
                GNCCL_IN_GROUP(g->api->Send(l.sendBuf, (size_t)l.nSend * sizeof(GhostRec), kNcclUint8, l.peerRank, g->comm, g->xstream));
            if (l.nRecv)
                GNCCL_IN_GROUP(g->api->Recv(l.recvBuf, (size_t)l.nRecv * sizeof(GhostRec), kNcclUint8, l.peerRank, g->comm, g->xstream));
        }
    }
#undef GNCCL_IN_GROUP
    GNCCL(g->api->GroupEnd());
    GHIP(hipEventRecord(g->evExchanged, g->xstream));
    const double t2 = now_us();
    g->hostUs[2] += t2 - t1;
    for (auto& s : g->slabs) {
        deme_ctx* c = s.ctx;
        GHIP(hipStreamWaitEvent(c->haloStream, g->evExchanged, 0));
        for (auto& sd : s.side)
            if (sd.peerRank >= 0 && sd.nRecv)
                hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(sd.nRecv)), dim3(256), 0, c->haloStream, sd.nRecv, (const uint32_t*)sd.recvIds,
                                   c->owners.as<OwnerRec>(), (const GhostRec*)sd.recvBuf);
        GHIP(hipEventRecord(c->evHaloDone, c->haloStream));
    }
    g->nExchanges++;
    g->hostUs[3] += now_us() - t2;
    return DEME_OK;
}

// ---- one evaluation per cross-cut contact ----------------------------------------------------------------------------------------
// By default a contact between an own clump and a ghost is evaluated on both ranks (each keeps a history copy, the force on the
// ghost is dropped).  With deme_halo_group_set_cross_contacts(g, 1) the LEFT slab of a cut evaluates it -- the right slab marks its
// left ghosts passive (OWNER_PASSIVE_BIT) and the sweep leaves their pairs with own clumps out, along with every ghost sphere's
// wall and mesh contacts -- and after its ghost-dependent force pass it sends a / alpha of each right ghost's contact sum to the
// ghost's owner, which adds them to the clump's own before integrating ("reverse exchange of the ghost's force").
static int rev_setup_slab(deme_halo_group* g, HaloSlab& s) {
    deme_ctx* c = s.ctx;
    c->crossStale = false;
    if (c->nOwners != s.nOwnersAtAttach)
        return gfail(g, DEME_ERR_INVALID, "cross contacts: the slab's scene changed size since it was attached (%u -> %u owners): its exchange "
                                          "lists are stale, attach it to a new group", s.nOwnersAtAttach, c->nOwners);
    c->pairsOnce = g->pairsOnce;
    c->dp.hasGhosts = (c->hasGhosts ? 1u : 0u) | (c->pairsOnce ? 2u : 0u);
    c->revAcc = nullptr;
    HaloSide &l = s.side[0], &r = s.side[1];
    if (l.peerRank >= 0 && l.nRecv)  // my left ghosts: passive or not
        hipLaunchKernelGGL(k_owner_set_bits, dim3(grid_for(l.nRecv)), dim3(256), 0, c->stream, l.nRecv, (const uint32_t*)l.recvIds,
                           c->owners.as<OwnerRec>(), (uint32_t)OWNER_PASSIVE_BIT, g->pairsOnce ? (uint32_t)OWNER_PASSIVE_BIT : 0u);
    c->listStale = true;  // the rule changes what belongs on the list
    if (!g->pairsOnce)
        return DEME_OK;
    if (!s.evRev)
        GHIP(hipEventCreateWithFlags(&s.evRev, hipEventDisableTiming));
    if (!g->evRevDone)
        GHIP(hipEventCreateWithFlags(&g->evRevDone, hipEventDisableTiming));
    const uint32_t want[2] = {l.peerRank >= 0 ? l.nSend : 0u, r.peerRank >= 0 ? r.nRecv : 0u};
    for (int k = 0; k < 2; k++) {
        HaloSide& sd = s.side[k];
        if (want[k] > sd.revCap) {
            if (sd.revBuf)
                GHIP(hipFree(sd.revBuf));
            sd.revCap = want[k] + want[k] / 4 + 64;
            GHIP(hipMalloc(&sd.revBuf, (size_t)sd.revCap * 32));
        }
    }
    if (ensure(c, c->revSlot, std::max<size_t>(c->nOwners, 1) * 4))
        return gfail(g, c->lastStatus, "cross contacts: %s", c->err.c_str());
    GHIP(hipMemsetAsync(c->revSlot.p, 0xFF, std::max<size_t>(c->nOwners, 1) * 4, c->stream));
    if (want[0]) {
        hipLaunchKernelGGL(k_rev_slots, dim3(grid_for(l.nSend)), dim3(256), 0, c->stream, l.nSend, (const uint32_t*)l.sendIds,
                           c->revSlot.as<uint32_t>());
        GHIP(hipMemsetAsync(l.revBuf, 0, (size_t)l.nSend * 32, c->stream));  // (nothing has been received yet)
        c->revAcc = l.revBuf;
    }
    return DEME_OK;
}

int deme_halo_group_set_cross_contacts(deme_halo_group* g, int evaluateOnce) {
    if (!g || !g->comm)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    if (evaluateOnce && g->nShared)
        return gfail(g, DEME_ERR_INVALID, "cross contacts: replicated free owners are summed over both evaluations of a cross-cut contact; not combined with the single evaluation yet");
    g->pairsOnce = evaluateOnce != 0;
    for (auto& s : g->slabs) {
        if (int rc = rev_setup_slab(g, s))
            return rc;
        GHIP(hipStreamSynchronize(s.ctx->stream));
    }
    return DEME_OK;
}

// after every slab's ghost-dependent force pass: pack the right ghosts' sums, one RCCL group (each cut: left slab -> right slab),
// the integrations wait for what they receive
// `waitNow` false: the compute streams are NOT made to wait here -- the caller integrates the owners that expect no share beside the
// exchange and waits on evRevDone before the ones that do (one_step)
static int reverse_exchange(deme_halo_group* g, bool waitNow = true) {
    auto find = [&](deme_ctx* c) -> HaloSlab* {
        for (auto& s : g->slabs)
            if (s.ctx == c)
                return &s;
        return nullptr;
    };
    for (auto& s : g->slabs) {
        deme_ctx* c = s.ctx;
        HaloSide& r = s.side[1];
        if (r.peerRank >= 0 && r.nRecv)
            hipLaunchKernelGGL(k_ghost_acc_pack, dim3(grid_for(r.nRecv)), dim3(256), 0, c->stream, c->dp, r.nRecv, (const uint32_t*)r.recvIds,
                               gather_args(c), c->owners.as<OwnerRec>(), (float4*)r.revBuf);
        GHIP(hipEventRecord(s.evRev, c->stream));
        GHIP(hipStreamWaitEvent(g->xstream, s.evRev, 0));
    }
    for (auto& s : g->slabs) {  // (checks before the group opens)
        HaloSide& r = s.side[1];
        if (r.peerRank >= 0 && r.peerLocal && !find(r.peerLocal))
            return gfail(g, DEME_ERR_INVALID, "a local neighbour context is not attached to the group");
    }
    GNCCL(g->api->GroupStart());
#define GNCCL_IN_GROUP(call)                                                                                                     \
    do {                                                                                                                         \
        int _r = (call);                                                                                                         \
        if (_r != 0) {                                                                                                           \
            g->api->GroupEnd();                                                                                                  \
            return gfail(g, DEME_ERR_HIP, "%s failed: %s (%s:%d)", #call, g->api->GetErrorString(_r), __FILE__, __LINE__);        \
        }                                                                                                                        \
    } while (0)
    for (auto& s : g->slabs) {
        HaloSide& r = s.side[1];
        if (r.peerRank >= 0 && r.nRecv) {
            if (r.peerLocal) {  // to self: the send right before the receive it feeds
                HaloSide& l = find(r.peerLocal)->side[0];
                GNCCL_IN_GROUP(g->api->Send(r.revBuf, (size_t)r.nRecv * 32, kNcclUint8, g->rank, g->comm, g->xstream));
                GNCCL_IN_GROUP(g->api->Recv(l.revBuf, (size_t)l.nSend * 32, kNcclUint8, g->rank, g->comm, g->xstream));
            } else {
                GNCCL_IN_GROUP(g->api->Send(r.revBuf, (size_t)r.nRecv * 32, kNcclUint8, r.peerRank, g->comm, g->xstream));
            }
        }
        HaloSide& l = s.side[0];
        if (l.peerRank >= 0 && !l.peerLocal && l.nSend)
            GNCCL_IN_GROUP(g->api->Recv(l.revBuf, (size_t)l.nSend * 32, kNcclUint8, l.peerRank, g->comm, g->xstream));
    }
#undef GNCCL_IN_GROUP
    GNCCL(g->api->GroupEnd());
    GHIP(hipEventRecord(g->evRevDone, g->xstream));
    if (waitNow)
        for (auto& s : g->slabs)
            GHIP(hipStreamWaitEvent(s.ctx->stream, g->evRevDone, 0));
    g->nRevExchanges++;
    return DEME_OK;
}

// Second half of a step when the scene has replicated free owners (a mesh or an analytical body that moves under contact forces,
// kept on every slab): every slab finishes its force passes and reduces its own spheres' contributions to those owners; the
// per-slab sums are added up -- first across the slabs of this process, in slab order, then across the ranks with one all-reduce --
// and every slab integrates its replica with the same total.  (the only all-reduce of the path.)
static int shared_tail(deme_halo_group* g) {
    const uint32_t n = g->nShared, n4 = 2 * n;
    for (auto& s : g->slabs)  // the rules would see each slab's PARTIAL acceleration of a replicated owner and could decide differently per slab
        if (s.ctx->rulesFn && s.ctx->rulesNeedAcc)
            return gfail(g, DEME_ERR_INVALID, "family-change rules that read accelerations cannot be combined with replicated free owners under decomposition");
    for (auto& s : g->slabs) {
        deme_ctx* c = s.ctx;
        if (int rc = overlap_forces(c))
            return gfail(g, rc, "step (boundary forces): %s", c->err.c_str());
        if (int rc = step_tail_pre(c))
            return gfail(g, rc, "step (reductions): %s", c->err.c_str());
        hipLaunchKernelGGL(k_shared_pack, dim3(grid_for(n4)), dim3(256), 0, c->stream, n, c->sharedIds.as<uint32_t>(), c->acc.as<AccRec>(),
                           c->sharedBuf.as<float4>());
        GHIP(hipEventRecord(s.evAcc, c->stream));
        GHIP(hipStreamWaitEvent(g->xstream, s.evAcc, 0));
    }
    GHIP(hipMemcpyAsync(g->sharedSum, g->slabs[0].ctx->sharedBuf.p, (size_t)n * sizeof(AccRec), hipMemcpyDeviceToDevice, g->xstream));
    for (size_t k = 1; k < g->slabs.size(); k++)
        hipLaunchKernelGGL(k_shared_add, dim3(grid_for(n4)), dim3(256), 0, g->xstream, n4, (float4*)g->sharedSum,
                           g->slabs[k].ctx->sharedBuf.as<float4>());
    GNCCL(g->api->AllReduce(g->sharedSum, g->sharedSum, (size_t)n * 8, kNcclFloat32, kNcclSum, g->comm, g->xstream));
    GHIP(hipEventRecord(g->evReduced, g->xstream));
    g->nReductions++;
    for (auto& s : g->slabs) {
        deme_ctx* c = s.ctx;
        GHIP(hipStreamWaitEvent(c->stream, g->evReduced, 0));
        hipLaunchKernelGGL(k_shared_unpack, dim3(grid_for(n4)), dim3(256), 0, c->stream, n, c->sharedIds.as<uint32_t>(), c->acc.as<AccRec>(),
                           (const float4*)g->sharedSum);
        if (int rc = step_tail_post(c))
            return gfail(g, rc, "step (integration): %s", c->err.c_str());
    }
    return DEME_OK;
}

// nsteps time steps of every slab this process holds, each with its ghost exchange: interior force pass on the compute streams
// while the records travel, the ghost-dependent pass and the integration after they have arrived.  Asynchronous like deme_step.
int deme_halo_group_step(deme_halo_group* g, uint32_t nsteps) {
    if (!g || !g->comm)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    auto one_step = [&]() -> int {
        const double t0 = now_us();
        for (auto& s : g->slabs)
            if (int rc = deme_step_overlap_begin(s.ctx, nullptr))
                return gfail(g, rc, "step (interior forces): %s", s.ctx->err.c_str());
        g->hostUs[0] += now_us() - t0;
        if (int rc = halo_exchange(g))
            return rc;
        const double t1 = now_us();
        if (g->pairsOnce) {
            for (auto& s : g->slabs)
                if (int rc = overlap_forces(s.ctx))
                    return gfail(g, rc, "step (boundary forces): %s", s.ctx->err.c_str());
            // The reactions travel while every slab integrates the owners that expect none (all but the clumps on its send-left
            // list); those are integrated when the share has arrived.  (Family rules that read accelerations see the complete sums
            // of every owner before anything is integrated: the unsplit order serves then.)
            static const int splitEnv = getenv("DEME_REV_SPLIT") ? atoi(getenv("DEME_REV_SPLIT")) : 1;
            bool split = splitEnv != 0;
            for (auto& s : g->slabs)
                if (s.ctx->rulesFn)
                    split = false;
            if (int rc = reverse_exchange(g, !split))
                return rc;
            if (!split) {
                for (auto& s : g->slabs)
                    if (int rc = step_tail(s.ctx))
                        return gfail(g, rc, "step (integration): %s", s.ctx->err.c_str());
            } else {
                for (auto& s : g->slabs) {
                    if (int rc = step_tail_pre(s.ctx))
                        return gfail(g, rc, "step (reductions): %s", s.ctx->err.c_str());
                    if (int rc = step_tail_post(s.ctx, Owners::NotWaiting))
                        return gfail(g, rc, "step (integration beside the reverse exchange): %s", s.ctx->err.c_str());
                }
                for (auto& s : g->slabs) {
                    const HaloSide& l = s.side[0];
                    GHIP(hipStreamWaitEvent(s.ctx->stream, g->evRevDone, 0));
                    const bool waits = l.peerRank >= 0 && l.nSend && s.ctx->revAcc;
                    if (int rc = step_tail_later(s.ctx, waits ? (const uint32_t*)l.sendIds : nullptr, waits ? l.nSend : 0u))
                        return gfail(g, rc, "step (integration of the clumps that waited for their share): %s", s.ctx->err.c_str());
                }
            }
        } else if (g->nShared == 0) {
            for (auto& s : g->slabs) {
                s.ctx->inGroupStep = true;
                const int rc = deme_step_overlap_end(s.ctx);
                s.ctx->inGroupStep = false;
                if (rc)
                    return gfail(g, rc, "step (boundary forces, integration): %s", s.ctx->err.c_str());
            }
        } else if (int rc = shared_tail(g)) {
            return rc;
        }
        g->hostUs[3] += now_us() - t1;
        return DEME_OK;
    };
    for (auto& s : g->slabs)  // a scene re-uploaded under the single-evaluation rule: passive marks and reaction slots again
        if (s.ctx->crossStale && g->pairsOnce)
            if (int rc = rev_setup_slab(g, s))
                return rc;
    auto clear_snap = [&]() {  // a failed step must not leave a snapshot request behind for the next call
        for (auto& s : g->slabs)
            s.ctx->snapPending = false;
    };
    for (uint32_t i = 0; i < nsteps; i++) {
        // asynchronous detection (deme_set_async_detection on the slabs' contexts): every slab decides for itself -- a detection
        // is local, the exchange of a step does not depend on it.  The slabs whose lists retire D steps from now take their owner
        // snapshot inside the next step (after its ghosts arrive), the D steps are enqueued -- exchanges included: everything is
        // stream-ordered --, and while the GPU works through them the host drives part 1 of those slabs on their detection streams.
        std::vector<deme_ctx*> starters;
        uint32_t D = 0;
        if (g->nShared == 0)
            for (auto& s : g->slabs)
                if (async_detection_can_start(s.ctx, nsteps - i) && (starters.empty() || s.ctx->asyncLead == D)) {
                    D = s.ctx->asyncLead;
                    starters.push_back(s.ctx);
                }
        if (!starters.empty()) {
            for (deme_ctx* c : starters)
                c->snapPending = true;
            for (uint32_t d = 0; d < D; d++)
                if (int rc = one_step()) {
                    clear_snap();
                    return rc;
                }
            std::vector<uint64_t> nC(starters.size(), 0);
            for (size_t k = 0; k < starters.size(); k++)
                if (int rc = async_part1(starters[k], &nC[k]))
                    return gfail(g, rc, "asynchronous detection: %s", starters[k]->err.c_str());
            for (size_t k = 0; k < starters.size(); k++)
                if (int rc = async_part2(starters[k], nC[k]))
                    return gfail(g, rc, "asynchronous detection: %s", starters[k]->err.c_str());
            i += D - 1;
            continue;
        }
        if (int rc = one_step())
            return rc;
    }
    return DEME_OK;
}

int deme_halo_group_exchange(deme_halo_group* g) {  // ghosts refreshed without a step (after uploads; tests)
    if (!g || !g->comm)
        return DEME_ERR_INVALID;
    GHIP(hipSetDevice(g->device));
    for (auto& s : g->slabs)
        if (s.ctx->evStepDone)
            GHIP(hipEventRecord(s.ctx->evStepDone, s.ctx->stream));
    if (int rc = halo_exchange(g))
        return rc;
    for (auto& s : g->slabs)
        GHIP(hipStreamWaitEvent(s.ctx->stream, s.ctx->evHaloDone, 0));
    return DEME_OK;
}

int deme_halo_group_sync(deme_halo_group* g) {
    if (!g)
        return DEME_ERR_INVALID;
    for (auto& s : g->slabs) {
        GHIP(hipStreamSynchronize(s.ctx->stream));
        if (s.ctx->haloStream)
            GHIP(hipStreamSynchronize(s.ctx->haloStream));
    }
    if (g->xstream)
        GHIP(hipStreamSynchronize(g->xstream));
    return DEME_OK;
}

int deme_halo_group_host_time(deme_halo_group* g, double us[4], int reset) {
    if (!g || !us)
        return DEME_ERR_INVALID;
    for (int k = 0; k < 4; k++) {
        us[k] = g->hostUs[k];
        if (reset)
            g->hostUs[k] = 0;
    }
    return DEME_OK;
}

int deme_halo_group_stats(const deme_halo_group* g, uint64_t* exchanges, uint64_t* bytesSentPerStep) {
    if (!g)
        return DEME_ERR_INVALID;
    if (exchanges)
        *exchanges = g->nExchanges;
    if (bytesSentPerStep)
        *bytesSentPerStep = g->bytesPerStep;
    return DEME_OK;
}

int deme_halo_group_comm_count(const deme_halo_group* g, int* ranks) {
    if (!g || !g->comm || !ranks)
        return DEME_ERR_INVALID;
    return g->api->CommCount(g->comm, ranks) == 0 ? DEME_OK : DEME_ERR_HIP;
}

#include "deme_migrate_host.inc"

int deme_get_counts(deme_ctx* c, DemeCounts* out) {
    if (!c || !out)
        return DEME_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    out->nContacts = c->nContacts;
    out->nPrevContacts = c->nPrev;
    out->nBinSphereTouches = c->nInc;
    out->nActiveBins = c->nActiveBins;
    out->nSteps = c->nSteps;
    out->nDetections = c->nDetections;
    out->maxSpheresInBin = c->maxInBin;
    out->lastStatus = c->lastStatus;
    return DEME_OK;
}

int deme_download_bin_incidence(deme_ctx* c, uint32_t* bins, uint32_t* sph, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    if (cap < c->nInc)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %llu", (unsigned long long)c->nInc);
    std::vector<uint32_t> hb;
    uint32_t* binsHost = bins;
    if (c->permuted && sph && !bins) {  // (the bins are needed to put each bin's spheres in the caller's order)
        hb.resize(c->nInc);
        binsHost = hb.data();
    }
    if (c->nInc) {
        if (binsHost)
            HIPCK(hipMemcpyAsync(binsHost, c->incKeys[1].p, c->nInc * 4, hipMemcpyDeviceToHost, c->stream));
        if (sph)
            HIPCK(hipMemcpyAsync(sph, c->incVals[1].p, c->nInc * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->permuted && sph) {  // caller's sphere ids, ascending within every bin
        for (size_t i = 0; i < c->nInc; i++)
            sph[i] = c->hS2E[sph[i]];
        for (size_t b = 0; b < c->nInc;) {
            size_t e = b + 1;
            while (e < c->nInc && binsHost[e] == binsHost[b])
                e++;
            std::sort(sph + b, sph + e);
            b = e;
        }
    }
    return DEME_OK;
}

int deme_download_contacts(deme_ctx* c, uint32_t* idA, uint32_t* idB, uint8_t* type, uint32_t* mapping, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    const size_t n = c->nContacts;
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    // the list in the caller's ids and canonical order (the engine's own when it keeps the caller's numbering)
    if (int rc = order_current_view(c))
        return rc;
    const std::vector<uint64_t>& k = c->viewKeys;
    if (mapping && n && c->seeded) {  // a seeded list (deme_seed_contacts, a renewed order) has no previous list to map to
        for (size_t i = 0; i < n; i++)
            mapping[i] = 0xFFFFFFFFu;
    } else if (mapping && n) {
        std::vector<uint32_t> m(n);
        HIPCK(hipMemcpyAsync(m.data(), c->list[c->cur].mapping.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        if (!c->permuted) {
            memcpy(mapping, m.data(), n * 4);
        } else {  // row i of the caller's view came from which row of the caller's view of the PREVIOUS list
            std::vector<uint64_t> pk;
            std::vector<uint32_t> pperm;
            if (int rc = order_view_of(c, c->keysSorted[c->keysCur ^ 1].as<uint64_t>(), c->nPrev, pk, pperm))
                return rc;
            std::vector<uint32_t> pinv(c->nPrev);
            for (size_t i = 0; i < c->nPrev; i++)
                pinv[pperm[i]] = (uint32_t)i;
            for (size_t i = 0; i < n; i++) {
                const uint32_t from = m[c->viewPerm[i]];
                mapping[i] = from < c->nPrev ? pinv[from] : from;
            }
        }
    }
    for (size_t i = 0; i < n; i++) {
        const uint32_t cls = key_class(k[i]);
        if (idA)
            idA[i] = key_a(k[i]);
        if (idB)
            idB[i] = key_b(k[i]);
        if (type) {
            if (cls == DEME_KEY_CLASS_SS)
                type[i] = DEME_SPHERE_SPHERE_CONTACT;
            else if (cls == DEME_KEY_CLASS_SM)
                type[i] = DEME_SPHERE_MESH_CONTACT;
            else
                type[i] = (c->hObjType[key_b(k[i])] == DEME_ANAL_OBJ_TYPE_PLANE) ? DEME_SPHERE_PLANE_CONTACT
                                                                                   : DEME_SPHERE_CYL_CONTACT;
        }
    }
    return DEME_OK;
}

int deme_download_contact_wildcard(deme_ctx* c, uint32_t w, float* out, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    const uint32_t nW = c->hp.nContactWildcards;
    if (w >= nW)
        return fail(c, DEME_ERR_INVALID, "wildcard %u out of range (%u)", w, nW);
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    const size_t n = c->nContacts;
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    std::vector<float> h(n * nW);
    if (n)
        HIPCK(hipMemcpyAsync(h.data(), c->wc[c->wcCur].p, n * nW * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->permuted) {  // rows in the caller's list order
        if (int rc = order_current_view(c))
            return rc;
        for (size_t i = 0; i < n; i++)
            out[i] = h[(size_t)c->viewPerm[i] * nW + w];
        return DEME_OK;
    }
    for (size_t i = 0; i < n; i++)
        out[i] = h[i * nW + w];
    return DEME_OK;
}

int deme_upload_contact_wildcard(deme_ctx* c, uint32_t w, const float* in, size_t n) {
    if (int rc = check_ready(c))
        return rc;
    const uint32_t nW = c->hp.nContactWildcards;
    if (w >= nW || n != c->nContacts)
        return fail(c, DEME_ERR_INVALID, "wildcard upload: index %u of %u, %zu values for %llu contacts", w, nW, n,
                    (unsigned long long)c->nContacts);
    if (c->mapFresh)
        if (int rc = do_migrate(c))
            return rc;
    std::vector<float> h(n * nW);
    if (n)
        HIPCK(hipMemcpyAsync(h.data(), c->wc[c->wcCur].p, n * nW * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->permuted)
        if (int rc = order_current_view(c))
            return rc;
    for (size_t i = 0; i < n; i++)
        h[(c->permuted ? (size_t)c->viewPerm[i] : i) * nW + w] = in[i];
    if (n)
        HIPCK(hipMemcpyAsync(c->wc[c->wcCur].p, h.data(), n * nW * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_seed_contacts(deme_ctx* c, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, const float* wildcards,
                       size_t n) {
    if (int rc = check_ready(c))
        return rc;
    const uint32_t nW = c->hp.nContactWildcards;
    if (n && (!idA || !idB || !type || (nW && !wildcards)))
        return fail(c, DEME_ERR_INVALID, "deme_seed_contacts: null input");
    std::vector<uint64_t> keys(n);
    std::vector<uint8_t> flip(n, 0);
    for (size_t i = 0; i < n; i++) {
        const uint64_t cls = key_class_of_type(type[i]);
        const uint32_t nB = (cls == DEME_KEY_CLASS_SS) ? c->dp.nSpheres : (cls == DEME_KEY_CLASS_SM) ? c->dp.nTri : c->dp.nAnal;
        if (idA[i] >= c->dp.nSpheres || idB[i] >= nB)
            return fail(c, DEME_ERR_INVALID, "deme_seed_contacts: pair %zu (%u, %u, type %u) is out of range", i, idA[i], idB[i],
                        (unsigned)type[i]);
        uint32_t a = idA[i], b = idB[i];
        if (cls == DEME_KEY_CLASS_SS) {
            if (a == b)
                return fail(c, DEME_ERR_INVALID, "deme_seed_contacts: pair %zu joins sphere %u to itself", i, a);
            if (a > b) {  // the sweep lists a sphere pair smaller id first (ss_key): a pair given the other way round is stored
                          // canonically, and the B-to-A vector history of the built-in model changes sign with the roles
                if (c->hp.forceModel == DEME_FORCE_CUSTOM && nW)
                    return fail(c, DEME_ERR_INVALID,
                                "deme_seed_contacts: pair %zu (%u, %u) must be given smaller sphere id first (the sign rule of a user "
                                "model's wildcards is not known to the library)", i, a, b);
                std::swap(a, b);
                flip[i] = 1;
            }
        }
        keys[i] = order_key_in(c, make_key(cls, a, b));  // (roles by the caller's ids; the engine's slots name the spheres)
    }
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; i++)
        perm[i] = (uint32_t)i;
    std::sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    std::vector<uint64_t> ks(n);
    std::vector<float> ws(n * (size_t)nW);
    for (size_t i = 0; i < n; i++) {
        ks[i] = keys[perm[i]];
        if (i && ks[i] == ks[i - 1])
            return fail(c, DEME_ERR_INVALID, "deme_seed_contacts: duplicate pair (%u, %u)", idA[perm[i]], idB[perm[i]]);
        for (uint32_t w = 0; w < nW; w++)
            ws[i * nW + w] = wildcards[(size_t)perm[i] * nW + w];
        if (flip[perm[i]] && c->hp.forceModel == DEME_FORCE_HERTZIAN)  // delta_tan_x/y/z (FullHertzianForceModel.cu) point B -> A
            for (uint32_t w = 0; w < 3 && w < nW; w++)
                ws[i * nW + w] = -ws[i * nW + w];
    }
    if (n > c->cntCap)
        if (int rc = grow_contact_arena(c, n + n / 4 + 1024))
            return rc;
    if (n) {
        HIPCK(hipMemcpyAsync(c->keysSorted[c->keysCur].p, ks.data(), n * 8, hipMemcpyHostToDevice, c->stream));
        if (nW)
            HIPCK(hipMemcpyAsync(c->wc[c->wcCur].p, ws.data(), n * nW * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    c->nContacts = n;
    c->listSerial++;
    c->nPrev = 0;
    c->nWcStored = n;
    c->haveList = true;
    c->seeded = true;
    c->mapFresh = false;
    c->conValid = false;
    c->list[c->cur].invalidate();
    return DEME_OK;
}

int deme_set_record_contacts(deme_ctx* c, int enable) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    c->record = enable != 0;
    if (c->record && c->cntCap)
        for (int k = 0; k < 4; k++)
            if (int rc = ensure(c, c->rec[k], c->cntCap * 12))
                return rc;
    return DEME_OK;
}

int deme_download_contact_records(deme_ctx* c, float* force, float* torqueOnly, float* cpA, float* cpB, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = records_refused(c))
        return rc;
    const size_t n = c->nContacts;
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    float* dst[4] = {force, torqueOnly, cpA, cpB};
    if (c->permuted) {
        if (int rc = order_current_view(c))
            return rc;
        std::vector<float> h(n * 3);
        for (int k = 0; k < 4; k++)
            if (dst[k] && n) {
                HIPCK(hipMemcpyAsync(h.data(), c->rec[k].p, n * 12, hipMemcpyDeviceToHost, c->stream));
                HIPCK(hipStreamSynchronize(c->stream));
                for (size_t i = 0; i < n; i++)
                    memcpy(dst[k] + 3 * i, h.data() + 3 * (size_t)c->viewPerm[i], 12);
            }
        return DEME_OK;
    }
    for (int k = 0; k < 4; k++)
        if (dst[k] && n)
            HIPCK(hipMemcpyAsync(dst[k], c->rec[k].p, n * 12, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_download_sphere_geometry(deme_ctx* c, double* X, double* Y, double* Z, float* R, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    const size_t n = c->nSpheres;
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    if (c->geoStale)
        return fail(c, DEME_ERR_INVALID, "the engine's order was renewed after the last detection: the sphere geometry of the new slots is computed by the next one");
    std::vector<GeoRec> h(n);
    if (n)
        HIPCK(hipMemcpyAsync(h.data(), c->geo.p, n * sizeof(GeoRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; k++) {
        const size_t i = order_sphere_out(c, (uint32_t)k);
        if (X) X[i] = h[k].x;
        if (Y) Y[i] = h[k].y;
        if (Z) Z[i] = h[k].z;
        if (R) R[i] = h[k].r;
    }
    return DEME_OK;
}

static size_t wc_array_len(deme_ctx* c, uint32_t kind) {
    return kind == 0 ? c->nOwners : kind == 1 ? c->nSpheres : kind == 2 ? c->nTri : c->nAnal;
}

int deme_compile_force_model_ex(deme_ctx* c, const char* src, size_t len, const char* const* wildcardNames, uint32_t nWildcards,
                                const char* const* ownerNames, uint32_t nOwnerWc, const char* const* geoNames, uint32_t nGeoWc,
                                const char* prerequisites) {
    if (!c || !src)
        return DEME_ERR_INVALID;
    if (!c->haveScene)
        return fail(c, DEME_ERR_INVALID, "upload the scene first: material tables are compiled into the model");
    if (nWildcards != c->hp.nContactWildcards)
        return fail(c, DEME_ERR_INVALID, "%u wildcard names given but DemeParams.nContactWildcards is %u", nWildcards,
                    c->hp.nContactWildcards);
    if (nOwnerWc > 8 || nGeoWc > 8)
        return fail(c, DEME_ERR_INVALID, "at most 8 owner and 8 geometry wildcards are supported");
    std::vector<std::string> names, onames, gnames;
    for (uint32_t i = 0; i < nWildcards; i++)
        names.emplace_back(wildcardNames[i] ? wildcardNames[i] : "");
    for (uint32_t i = 0; i < nOwnerWc; i++)
        onames.emplace_back(ownerNames[i] ? ownerNames[i] : "");
    for (uint32_t i = 0; i < nGeoWc; i++)
        gnames.emplace_back(geoNames[i] ? geoNames[i] : "");
    std::string gen, err;
    if (deme_jit::generate_source(std::string(src, len), names, prerequisites ? prerequisites : "", c->mt, gen, err, onames, gnames))
        return fail(c, DEME_ERR_COMPILE, "%s", err.c_str());
    const size_t key = std::hash<std::string>{}(gen);
    auto it = c->jitCache.find(key);
    if (it == c->jitCache.end()) {
        std::vector<char> code;
        std::string log;
        if (deme_jit::compile(gen, code, log))
            return fail(c, DEME_ERR_COMPILE, "force model failed to compile:\n%.900s", log.c_str());
        it = c->jitCache.emplace(key, std::move(code)).first;
    }
    HIPCK(hipStreamSynchronize(c->stream));
    // wildcard arrays: existing ones keep their values, new ones start at zero
    for (uint32_t kind = 0; kind < 4; kind++) {
        const uint32_t want = kind == 0 ? nOwnerWc : nGeoWc;
        const size_t n = wc_array_len(c, kind);
        for (uint32_t k = 0; k < want; k++)
            if (!c->userWc[kind][k].p && n) {
                if (int rc = ensure(c, c->userWc[kind][k], n * 4))
                    return rc;
                HIPCK(hipMemsetAsync(c->userWc[kind][k].p, 0, n * 4, c->stream));
            }
    }
    c->nOwnerWc = nOwnerWc, c->nGeoWc = nGeoWc;
    if (c->customMod) {
        (void)hipModuleUnload(c->customMod);
        c->customMod = nullptr;
        c->customFn[0] = c->customFn[1] = c->customFn[2] = nullptr;
        c->customTileFn[0] = c->customTileFn[1] = c->customTileFn[2] = c->customTileFn[3] = nullptr;
    }
    HIPCK(hipModuleLoadData(&c->customMod, it->second.data()));
    HIPCK(hipModuleGetFunction(&c->customFn[0], c->customMod, "deme_custom_forces_ss"));
    HIPCK(hipModuleGetFunction(&c->customFn[1], c->customMod, "deme_custom_forces_sm"));
    bool tileAll = true;
    for (int k = 0; k < 4; k++)
        if (hipModuleGetFunction(&c->customTileFn[k], c->customMod, deme_jit::kTileEntry[k]) != hipSuccess)
            tileAll = false;
    if (!tileAll)  // all four (tile / big-tile fallback, with and without mesh records) or none: a list with a tile that does not fit
                   // LDS, or a scene with a mesh, must never find its entry missing -- the general kernel evaluates the lists then
        c->customTileFn[0] = c->customTileFn[1] = c->customTileFn[2] = c->customTileFn[3] = nullptr;
    c->listStale = true;  // the list structures depend on which kernel evaluates the list
    return DEME_OK;
}

int deme_compile_force_model(deme_ctx* c, const char* src, size_t len, const char* const* wildcardNames, uint32_t nWildcards,
                             const char* prerequisites) {
    return deme_compile_force_model_ex(c, src, len, wildcardNames, nWildcards, nullptr, 0, nullptr, 0, prerequisites);
}

int deme_upload_wildcard_array(deme_ctx* c, uint32_t kind, uint32_t index, const float* in, size_t n) {
    if (int rc = check_ready(c))
        return rc;
    if (kind > 3 || index >= 8 || !in)
        return fail(c, DEME_ERR_INVALID, "wildcard array: kind %u index %u", kind, index);
    if (n != wc_array_len(c, kind))
        return fail(c, DEME_ERR_INVALID, "wildcard array of kind %u holds %zu values, %zu given", kind, wc_array_len(c, kind), n);
    if (int rc = ensure(c, c->userWc[kind][index], std::max<size_t>(n, 1) * 4))
        return rc;
    // (owner and sphere wildcard arrays are indexed by the ids user code sees -- the caller's -- and stay in the caller's order
    // whatever order the engine keeps the owners in: deme_order.inc)
    if (n)
        HIPCK(hipMemcpyAsync(c->userWc[kind][index].p, in, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_download_wildcard_array(deme_ctx* c, uint32_t kind, uint32_t index, float* out, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    if (kind > 3 || index >= 8 || !out || !c->userWc[kind][index].p)
        return fail(c, DEME_ERR_INVALID, "wildcard array: kind %u index %u does not exist", kind, index);
    const size_t n = wc_array_len(c, kind);
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    if (n)
        HIPCK(hipMemcpyAsync(out, c->userWc[kind][index].p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_compile_prescriptions(deme_ctx* c, const char* velCases, const char* posCases, const char* accCases) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->prescMod) {
        (void)hipModuleUnload(c->prescMod);
        c->prescMod = nullptr;
        c->prescFn = nullptr;
    }
    c->prescDirty = true;
    const std::string v = velCases ? velCases : "", ps = posCases ? posCases : "", a = accCases ? accCases : "";
    if (v.empty() && ps.empty() && a.empty())
        return DEME_OK;
    std::string gen;
    deme_jit::generate_prescribe_source(v, ps, a, gen);
    const size_t key = std::hash<std::string>{}(gen);
    auto it = c->jitCache.find(key);
    if (it == c->jitCache.end()) {
        std::vector<char> code;
        std::string log;
        if (deme_jit::compile(gen, code, log))
            return fail(c, DEME_ERR_COMPILE, "family prescriptions failed to compile:\n%.900s", log.c_str());
        it = c->jitCache.emplace(key, std::move(code)).first;
    }
    HIPCK(hipModuleLoadData(&c->prescMod, it->second.data()));
    HIPCK(hipModuleGetFunction(&c->prescFn, c->prescMod, "deme_prescribe"));
    return DEME_OK;
}

int deme_compile_family_rules(deme_ctx* c, const char* rules) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->rulesMod) {
        (void)hipModuleUnload(c->rulesMod);
        c->rulesMod = nullptr;
        c->rulesFn = nullptr;
    }
    c->prescDirty = true;
    const std::string r = rules ? rules : "";
    if (r.find_first_not_of(" \t\n") == std::string::npos)
        return DEME_OK;
    // whole-word scan for the contact acceleration, as the reference scans force models for their ingredients
    auto mentions = [&](const std::string& w) {
        for (size_t pos = r.find(w); pos != std::string::npos; pos = r.find(w, pos + 1)) {
            const bool l = pos == 0 || !(isalnum((unsigned char)r[pos - 1]) || r[pos - 1] == '_');
            const size_t e = pos + w.size();
            const bool rr = e >= r.size() || !(isalnum((unsigned char)r[e]) || r[e] == '_');
            if (l && rr)
                return true;
        }
        return false;
    };
    c->rulesNeedAcc = mentions("acc") || mentions("accX") || mentions("accY") || mentions("accZ");
    std::string gen;
    deme_jit::generate_family_rules_source(r, gen);
    const size_t key = std::hash<std::string>{}(gen);
    auto it = c->jitCache.find(key);
    if (it == c->jitCache.end()) {
        std::vector<char> code;
        std::string log;
        if (deme_jit::compile(gen, code, log))
            return fail(c, DEME_ERR_COMPILE, "family change rules failed to compile:\n%.900s", log.c_str());
        it = c->jitCache.emplace(key, std::move(code)).first;
    }
    HIPCK(hipModuleLoadData(&c->rulesMod, it->second.data()));
    HIPCK(hipModuleGetFunction(&c->rulesFn, c->rulesMod, "deme_family_changes"));
    return DEME_OK;
}

int deme_add_owner_acc(deme_ctx* c, uint32_t owner, uint32_t n, const float* acc, const float* angAcc) {
    if (int rc = check_ready(c))
        return rc;
    if ((uint64_t)owner + n > c->nOwners || (!acc && !angAcc))
        return fail(c, DEME_ERR_INVALID, "deme_add_owner_acc: owners [%u, %u) out of range or nothing to set", owner, owner + n);
    if (c->hNextAcc.size() != c->nOwners) {
        c->hNextAcc.resize(c->nOwners);
        if (int rc = ensure(c, c->nextAcc, std::max<size_t>(c->nOwners, 1) * sizeof(AccRec)))
            return rc;
        if (int rc = zero_next_acc(c))
            return rc;
    }
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t slot = order_owner_in(c, owner + k);
        AccRec& r = c->hNextAcc[slot];
        if (acc)
            r.ax = acc[3 * k], r.ay = acc[3 * k + 1], r.az = acc[3 * k + 2];
        if (angAcc)
            r.lx = angAcc[3 * k], r.ly = angAcc[3 * k + 1], r.lz = angAcc[3 * k + 2];
        lo = std::min(lo, slot), hi = std::max(hi, slot + 1u);
    }
    if (n)  // one copy of the touched range of slots (the caller's range is not a range of slots on a reordered context: the host
            // mirror holds every record, so what lies between the touched ones is written back unchanged)
        HIPCK(hipMemcpyAsync(c->nextAcc.as<AccRec>() + lo, c->hNextAcc.data() + lo, (size_t)(hi - lo) * sizeof(AccRec),
                             hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->nextAccPending = true;
    return DEME_OK;
}

int deme_mark_persistent_contacts(deme_ctx* c, int mode, uint32_t N1, uint32_t N2, int mark) {
    if (int rc = check_ready(c))
        return rc;
    if (mode < 0 || mode > 3)
        return fail(c, DEME_ERR_INVALID, "deme_mark_persistent_contacts: mode %d is not one of 0 (all), 1 (either), 2 (both), 3 (pair)", mode);
    if (c->hp.nContactWildcards == 0)  // DEM/APIPrivate.cpp:38-43
        return fail(c, DEME_ERR_INVALID,
                    "persistent contacts cannot be marked with a history-less force model (persistency is part of the history); add a placeholder wildcard");
    const size_t nC = c->haveList ? c->nContacts : 0;
    std::vector<uint64_t> hit;
    if (nC) {
        if (int rc = ensure(c, c->stage, nC))
            return rc;
        hipLaunchKernelGGL(k_persist_flags, dim3(grid_for(nC)), dim3(256), 0, c->stream, c->dp, (uint32_t)nC,
                           c->keysSorted[c->keysCur].as<uint64_t>(), c->spheres.as<SphereRec>(), c->owners.as<OwnerRec>(), mode, N1, N2,
                           c->stage.as<uint8_t>());
        std::vector<uint8_t> flag(nC);
        std::vector<uint64_t> keys(nC);
        HIPCK(hipMemcpyAsync(flag.data(), c->stage.p, nC, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(keys.data(), c->keysSorted[c->keysCur].p, nC * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < nC; i++)
            if (flag[i])
                hit.push_back(keys[i]);  // ascending already
    }
    std::vector<uint64_t> out;
    if (mark)
        std::set_union(c->hPersist.begin(), c->hPersist.end(), hit.begin(), hit.end(), std::back_inserter(out));
    else
        std::set_difference(c->hPersist.begin(), c->hPersist.end(), hit.begin(), hit.end(), std::back_inserter(out));
    c->hPersist.swap(out);
    if (!c->hPersist.empty()) {
        if (int rc = ensure(c, c->persistKeys, c->hPersist.size() * 8))
            return rc;
        HIPCK(hipMemcpyAsync(c->persistKeys.p, c->hPersist.data(), c->hPersist.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    return DEME_OK;
}

int deme_download_persistent_contacts(deme_ctx* c, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    const size_t n = c->hPersist.size();
    if (cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    std::vector<uint64_t> keys(c->hPersist);
    if (c->permuted) {
        for (auto& k : keys)
            k = order_key_out(c, k);
        std::sort(keys.begin(), keys.end());
    }
    for (size_t i = 0; i < n; i++) {
        const uint64_t k = keys[i];
        const uint32_t cls = key_class(k);
        if (idA)
            idA[i] = key_a(k);
        if (idB)
            idB[i] = key_b(k);
        if (type)
            type[i] = cls == DEME_KEY_CLASS_SS   ? DEME_SPHERE_SPHERE_CONTACT
                      : cls == DEME_KEY_CLASS_SM ? DEME_SPHERE_MESH_CONTACT
                      : (c->hObjType[key_b(k)] == DEME_ANAL_OBJ_TYPE_PLANE ? DEME_SPHERE_PLANE_CONTACT : DEME_SPHERE_CYL_CONTACT);
    }
    return DEME_OK;
}

int deme_upload_persistent_contacts(deme_ctx* c, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, size_t n) {
    if (int rc = check_ready(c))
        return rc;
    if (n && (!idA || !idB || !type))
        return fail(c, DEME_ERR_INVALID, "deme_upload_persistent_contacts: null input");
    if (n && c->hp.nContactWildcards == 0)
        return fail(c, DEME_ERR_INVALID, "persistent contacts cannot be marked with a history-less force model");
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) {
        const uint64_t cls = key_class_of_type(type[i]);
        const uint32_t nB = (cls == DEME_KEY_CLASS_SS) ? c->dp.nSpheres : (cls == DEME_KEY_CLASS_SM) ? c->dp.nTri : c->dp.nAnal;
        if (idA[i] >= c->dp.nSpheres || idB[i] >= nB)
            return fail(c, DEME_ERR_INVALID, "deme_upload_persistent_contacts: pair %zu (%u, %u, type %u) is out of range", i, idA[i],
                        idB[i], (unsigned)type[i]);
        keys[i] = order_key_in(c, make_key(cls, idA[i], idB[i]));
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    c->hPersist.swap(keys);
    if (!c->hPersist.empty()) {
        if (int rc = ensure(c, c->persistKeys, c->hPersist.size() * 8))
            return rc;
        HIPCK(hipMemcpyAsync(c->persistKeys.p, c->hPersist.data(), c->hPersist.size() * 8, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
    }
    return DEME_OK;
}

int deme_num_persistent_contacts(deme_ctx* c, size_t* n) {
    if (!c || !n)
        return DEME_ERR_INVALID;
    *n = c->hPersist.size();
    return DEME_OK;
}

int deme_change_family(deme_ctx* c, uint32_t from, uint32_t to) {
    if (int rc = check_ready(c))
        return rc;
    if (from > 255 || to > 255)
        return fail(c, DEME_ERR_INVALID, "family numbers must not be larger than 255");
    if (c->nOwners)
        hipLaunchKernelGGL(k_change_family, dim3(grid_for(c->nOwners)), dim3(256), 0, c->stream, c->owners.as<OwnerRec>(),
                           (uint32_t)c->nOwners, from, to);
    c->prescDirty = true;
    c->listStale = true;  // pairs may have become unmasked
    return DEME_OK;
}

int deme_set_family_material(deme_ctx* c, uint32_t family, uint32_t material, int kind) {
    if (int rc = check_ready(c))
        return rc;
    if (family > 255 || material >= c->nMat || (kind != 0 && kind != 1))
        return fail(c, DEME_ERR_INVALID, "deme_set_family_material: family %u, material %u of %u, kind %d", family, material, c->nMat, kind);
    if (kind == 0 && c->nSpheres)
        hipLaunchKernelGGL(k_family_material_spheres, dim3(grid_for(c->nSpheres)), dim3(256), 0, c->stream, c->nSpheres,
                           c->spheres.as<SphereRec>(), c->owners.as<OwnerRec>(), family, material);
    if (kind == 1 && c->nTri)
        hipLaunchKernelGGL(k_family_material_tris, dim3(grid_for(c->nTri)), dim3(256), 0, c->stream, c->nTri, c->tris.as<TriRec>(),
                           c->owners.as<OwnerRec>(), family, material);
    c->listStale = true;  // the per-contact gather records hold the materials
    return DEME_OK;
}

int deme_device_memory(deme_ctx* c, size_t* usedBytes, size_t* totalBytes) {
    if (!c)
        return DEME_ERR_INVALID;
    size_t fr = 0, tot = 0;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipMemGetInfo(&fr, &tot));
    if (usedBytes)
        *usedBytes = tot - fr;
    if (totalBytes)
        *totalBytes = tot;
    return DEME_OK;
}

int deme_jit_probe_ex(const char* src, const char* const* wildcardNames, uint32_t nWildcards, const char* const* ownerNames,
                      uint32_t nOwnerWc, const char* const* geoNames, uint32_t nGeoWc, const char* prerequisites, char* log, size_t logCap) {
    deme_jit::MaterialTables mt;
    mt.nMat = 2;
    mt.E = {1e8f, 1e9f}, mt.nu = {0.3f, 0.3f};
    mt.CoR = {0.5f, 0.6f, 0.6f, 0.7f}, mt.mu = {0.2f, 0.3f, 0.3f, 0.4f}, mt.Crr = {0.f, 0.f, 0.f, 0.f};
    std::vector<std::string> names, onames, gnames;
    for (uint32_t i = 0; i < nWildcards; i++)
        names.emplace_back(wildcardNames[i] ? wildcardNames[i] : "");
    for (uint32_t i = 0; i < nOwnerWc; i++)
        onames.emplace_back(ownerNames[i] ? ownerNames[i] : "");
    for (uint32_t i = 0; i < nGeoWc; i++)
        gnames.emplace_back(geoNames[i] ? geoNames[i] : "");
    std::string gen, err, clog;
    std::vector<char> code;
    int rc = deme_jit::generate_source(src ? src : "", names, prerequisites ? prerequisites : "", mt, gen, err, onames, gnames);
    if (!rc) {
        rc = deme_jit::compile(gen, code, clog);
        err = clog;
    }
    if (log && logCap) {
        snprintf(log, logCap, "%s", err.c_str());
    }
    return rc ? DEME_ERR_COMPILE : DEME_OK;
}

int deme_jit_probe(const char* src, const char* const* wildcardNames, uint32_t nWildcards, const char* prerequisites,
                   char* log, size_t logCap) {
    return deme_jit_probe_ex(src, wildcardNames, nWildcards, nullptr, 0, nullptr, 0, prerequisites, log, logCap);
}

int deme_set_timing(deme_ctx* c, int enable) {
    if (!c)
        return DEME_ERR_INVALID;
    c->timing = enable > 0 ? enable : 0;
    return DEME_OK;
}
int deme_kernel_time_reset(deme_ctx* c) {
    if (!c)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (auto& kv : c->timers) {
        kv.second.total_ms = 0;
        kv.second.launches = 0;
        kv.second.seen = 0;
    }
    return DEME_OK;
}
namespace {
struct FMax {
    __host__ __device__ float operator()(float a, float b) const { return a > b ? a : b; }
};
struct FMin {
    __host__ __device__ float operator()(float a, float b) const { return a < b ? a : b; }
};
// fills c->stage with the per-element quantity; returns the element count through n.  region >= 0: elements outside the
// compiled region (deme_compile_region) get `identity`
int inspect_fill(deme_ctx* c, uint32_t q, float identity, size_t& n, int region = -1) {
    if (q > DEME_INSPECT_CLUMP_VOLUME)
        return fail(c, DEME_ERR_INVALID, "unknown inspection quantity %u", q);
    if (region >= (int)c->regionFn.size())
        return fail(c, DEME_ERR_INVALID, "unknown inspection region %d", region);
    if (q == DEME_INSPECT_CLUMP_VOLUME && !c->haveVolumes)
        return fail(c, DEME_ERR_INVALID, "clump_volume needs the templates' volumes (deme_upload_volumes)");
    const bool perSphere = q <= DEME_INSPECT_CLUMP_MAX_ABSV;
    n = perSphere ? c->nSpheres : c->nOwners;
    if (int rc = ensure(c, c->stage, std::max<size_t>(n, 1) * 4 + 16))
        return rc;
    if (n == 0)
        return DEME_OK;
    if (perSphere)
        hipLaunchKernelGGL(k_inspect_sphere, dim3(grid_for(n)), dim3(256), 0, c->stream, c->dp, c->owners.as<OwnerRec>(),
                           c->spheres.as<SphereRec>(), q, identity, c->stage.as<float>());
    else
        hipLaunchKernelGGL(k_inspect_owner, dim3(grid_for(n)), dim3(256), 0, c->stream, c->dp, c->owners.as<OwnerRec>(),
                           (uint32_t)c->nOwnerClumps, q, identity, c->volumes.as<float>(), c->stage.as<float>());
    if (region >= 0) {
        DevParams dp = c->dp;
        const OwnerRec* owners = c->owners.as<OwnerRec>();
        const SphereRec* spheres = c->spheres.as<SphereRec>();
        uint32_t nn = (uint32_t)n, ps = perSphere ? 1u : 0u;
        float* values = c->stage.as<float>();
        void* args[] = {&dp, &owners, &spheres, &nn, &ps, &identity, &values};
        HIPCK(hipModuleLaunchKernel(c->regionFn[region], grid_for(n), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
    }
    return DEME_OK;
}
}  // namespace

int deme_inspect_region(deme_ctx* c, uint32_t q, int region, float* out) {
    if (int rc = check_ready(c))
        return rc;
    if (!out || q == DEME_INSPECT_ABSV)
        return fail(c, DEME_ERR_INVALID, "deme_inspect: quantity %u has no reduction (use deme_inspect_values)", q);
    const bool isMax = q == DEME_INSPECT_CLUMP_MAX_Z || q == DEME_INSPECT_CLUMP_MAX_ABSV || q == DEME_INSPECT_MAX_ABSV;
    const bool isMin = q == DEME_INSPECT_CLUMP_MIN_Z;
    const float identity = isMax ? -3.402823466e38f : isMin ? 3.402823466e38f : 0.f;
    size_t n = 0;
    if (int rc = inspect_fill(c, q, identity, n, region))
        return rc;
    float* in = c->stage.as<float>();
    float* res = in + n;  // one spare slot behind the values
    if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
            return isMax   ? rocprim::reduce(tmp, bytes, in, res, identity, n, FMax(), c->stream)
                   : isMin ? rocprim::reduce(tmp, bytes, in, res, identity, n, FMin(), c->stream)
                           : rocprim::reduce(tmp, bytes, in, res, identity, n, rocprim::plus<float>(), c->stream);
        }))
        return rc;
    HIPCK(hipMemcpyAsync(out, res, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

int deme_inspect(deme_ctx* c, uint32_t q, float* out) { return deme_inspect_region(c, q, -1, out); }

int deme_compile_region(deme_ctx* c, const char* code, int* regionId) {
    if (!c || !regionId)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    const std::string r = code ? code : "";
    auto word = [&](const std::string& w) {
        for (size_t pos = r.find(w); pos != std::string::npos; pos = r.find(w, pos + 1)) {
            const bool l = pos == 0 || !(isalnum((unsigned char)r[pos - 1]) || r[pos - 1] == '_');
            const size_t e = pos + w.size();
            const bool rr = e >= r.size() || !(isalnum((unsigned char)r[e]) || r[e] == '_');
            if (l && rr)
                return true;
        }
        return false;
    };
    if (!(word("X") || word("Y") || word("Z")) || !word("return"))  // DEM/AuxClasses.cpp:209-219
        return fail(c, DEME_ERR_INVALID,
                    "an inspection region must return a bool that is a result of logical operations involving X, Y and Z");
    std::string gen;
    deme_jit::generate_region_source(r, gen);
    const size_t key = std::hash<std::string>{}(gen);
    auto it = c->jitCache.find(key);
    if (it == c->jitCache.end()) {
        std::vector<char> bin;
        std::string log;
        if (deme_jit::compile(gen, bin, log))
            return fail(c, DEME_ERR_COMPILE, "inspection region failed to compile:\n%.900s", log.c_str());
        it = c->jitCache.emplace(key, std::move(bin)).first;
    }
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    HIPCK(hipModuleLoadData(&mod, it->second.data()));
    HIPCK(hipModuleGetFunction(&fn, mod, "deme_region_filter"));
    c->regionMod.push_back(mod);
    c->regionFn.push_back(fn);
    *regionId = (int)c->regionFn.size() - 1;
    return DEME_OK;
}

int deme_upload_volumes(deme_ctx* c, const float* volumes, size_t n) {
    if (int rc = check_ready(c))
        return rc;
    if (!volumes || n != c->nMassProps)
        return fail(c, DEME_ERR_INVALID, "deme_upload_volumes: expected %u values (one per mass-property entry)", c->nMassProps);
    if (int rc = ensure(c, c->volumes, std::max<size_t>(n, 1) * 4))
        return rc;
    HIPCK(hipMemcpyAsync(c->volumes.p, volumes, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->haveVolumes = true;
    return DEME_OK;
}

int deme_inspect_values(deme_ctx* c, uint32_t q, float* out, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    size_t n = 0;
    if (int rc = inspect_fill(c, q, 0.f, n))
        return rc;
    if (!out || cap < n)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    if (n)
        HIPCK(hipMemcpyAsync(out, c->stage.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (c->permuted && n) {  // per sphere or per owner: back into the caller's numbering
        const std::vector<uint32_t>& m = n == c->nSpheres && n != c->nOwners ? c->hS2E : (q <= DEME_INSPECT_CLUMP_MAX_ABSV ? c->hS2E : c->hO2E);
        std::vector<float> tmp(out, out + n);
        for (size_t k = 0; k < n; k++)
            out[m[k]] = tmp[k];
    }
    return DEME_OK;
}

int deme_kernel_time_ms(deme_ctx* c, const char* name, double* avg_ms, uint64_t* launches) {
    if (!c || !name)
        return DEME_ERR_INVALID;
    hipSetDevice(c->device);  // (a process may hold contexts on several devices: deme_multi)
    hipStreamSynchronize(c->stream);
    drain_timers(c);
    auto it = c->timers.find(name);
    const double tot = it == c->timers.end() ? 0.0 : it->second.total_ms;
    const uint64_t n = it == c->timers.end() ? 0 : it->second.launches;
    if (avg_ms)
        *avg_ms = n ? tot / (double)n : 0.0;
    if (launches)
        *launches = n;
    return DEME_OK;
}

int deme_halo_pack(deme_ctx* c, const uint32_t* d_ids, uint32_t n, void* d_buf) {
    if (int rc = check_ready(c))
        return rc;
    if (n)
        hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n)), dim3(256), 0, c->stream, n, d_ids, c->owners.as<OwnerRec>(),
                           (GhostRec*)d_buf);
    return DEME_OK;
}
int deme_halo_unpack(deme_ctx* c, const uint32_t* d_ids, uint32_t n, const void* d_buf) {
    if (int rc = check_ready(c))
        return rc;
    if (n)
        hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(n)), dim3(256), 0, c->stream, n, d_ids, c->owners.as<OwnerRec>(),
                           (const GhostRec*)d_buf);
    return DEME_OK;
}

}  // extern "C"

// (templates inside: after the extern "C" block; its entry points take C linkage from their declarations in deme_hip.h)
// ---- run-time resizing of clumps (deme_resize.h) ------------------------------------------------------------------------------
namespace {
struct CompBits {  // a component's bit pattern: derived entries are shared by every sphere whose geometry is the same
    uint32_t w[4];
    bool operator<(const CompBits& o) const { return std::lexicographical_compare(w, w + 4, o.w, o.w + 4); }
};
CompBits comp_bits(const float4& v) {
    CompBits b;
    memcpy(&b.w[0], &v.x, 4), memcpy(&b.w[1], &v.y, 4), memcpy(&b.w[2], &v.z, 4), memcpy(&b.w[3], &v.w, 4);
    return b;
}
}  // namespace

// the checks every request passes before anything changes (the reference writes in place and races on a repeated id); fb: the
// factors' bits (a positive finite float has non-zero bits: 0 marks an owner that is not resized)
static int resize_check(char* msg, size_t cap, const uint32_t* ids, const float* factors, size_t n, uint32_t nOwners, std::vector<uint32_t>& fb) {
    if (n && (!ids || !factors))
        return snprintf(msg, cap, "null id or factor array"), DEME_ERR_INVALID;
    std::vector<uint8_t> seen(nOwners, 0);
    fb.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t o = ids[i];
        const float f = factors[i];
        if (o >= nOwners)
            return snprintf(msg, cap, "owner id %u is out of range (%u owners)", o, nOwners), DEME_ERR_INVALID;
        if (seen[o])
            return snprintf(msg, cap, "owner id %u is given twice", o), DEME_ERR_INVALID;
        if (!std::isfinite(f) || !(f > 0.f))
            return snprintf(msg, cap, "the factor of owner %u is %g; factors must be finite and > 0", o, (double)f), DEME_ERR_INVALID;
        seen[o] = 1;
        memcpy(&fb[i], &f, 4);
    }
    return DEME_OK;
}

// phase 1 (device): mark the owners (ids in this context's caller numbering), emit the keys of their spheres, count every
// component's uses; the distinct keys, how many spheres carry each, and the use counts come back to the host
static int resize_collect(deme_ctx* c, const uint32_t* ids, const uint32_t* fb, size_t n, std::vector<uint64_t>& keys,
                          std::vector<uint32_t>& runs, std::vector<uint32_t>& uses) {
    const uint32_t nS = c->nSpheres, nC = c->nComp;
    keys.clear(), runs.clear(), uses.assign(nC, 0);
    if (ensure(c, c->rsMark, (size_t)c->nOwners * 4 + 4) || ensure(c, c->rsKeys[0], (size_t)nS * 8 + 8) ||
        ensure(c, c->rsKeys[1], (size_t)nS * 8 + 8) || ensure(c, c->rsRuns, (size_t)nS * 4 + 16) || ensure(c, c->rsUses, (size_t)nC * 4 + 4) ||
        ensure(c, c->stage, n * 8 + 8))
        return c->lastStatus;
    uint32_t* dCnt = c->rsRuns.as<uint32_t>() + nS;  // [0]: keys emitted, [1]: distinct keys
    HIPCK(hipMemsetAsync(c->rsMark.p, 0, (size_t)c->nOwners * 4, c->stream));
    HIPCK(hipMemsetAsync(dCnt, 0, 8, c->stream));
    HIPCK(hipMemsetAsync(c->rsUses.p, 0, (size_t)nC * 4, c->stream));
    if (n) {
        uint32_t* dIds = c->stage.as<uint32_t>();
        uint32_t* dBits = dIds + n;
        HIPCK(hipMemcpyAsync(dIds, ids, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(dBits, fb, n * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_resize_mark, dim3(grid_for(n)), dim3(256), 0, c->stream, (uint32_t)n, dIds, dBits, c->rsMark.as<uint32_t>());
    }
    if (nS) {
        hipLaunchKernelGGL(k_resize_keys, dim3(grid_for(nS)), dim3(256), 0, c->stream, nS, c->spheres.as<SphereRec>(), c->dp.o2e,
                           c->rsMark.as<uint32_t>(), c->rsKeys[0].as<uint64_t>(), dCnt);
        hipLaunchKernelGGL(k_resize_uses, dim3(grid_for(nS)), dim3(256), 0, c->stream, nS, c->spheres.as<SphereRec>(), c->rsUses.as<uint32_t>());
    }
    uint32_t nK = 0;
    HIPCK(hipMemcpyAsync(&nK, dCnt, 4, hipMemcpyDeviceToHost, c->stream));
    if (nC)
        HIPCK(hipMemcpyAsync(uses.data(), c->rsUses.p, (size_t)nC * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    if (!nK)
        return DEME_OK;
    uint64_t* kIn = c->rsKeys[0].as<uint64_t>();
    uint64_t* kSorted = c->rsKeys[1].as<uint64_t>();
    uint32_t* runLen = c->rsRuns.as<uint32_t>();
    // (a key holds 48 bits: the 16-bit component index above the 32 factor bits)
    if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, kIn, kSorted, (size_t)nK, 0, 48, c->stream);
        }))
        return rc;
    if (int rc = with_temp(c, c->sortTmp, [&](void* tmp, size_t& bytes) {
            return rocprim::run_length_encode(tmp, bytes, kSorted, (size_t)nK, kIn, runLen, dCnt + 1, c->stream);
        }))
        return rc;
    uint32_t nU = 0;
    HIPCK(hipMemcpyAsync(&nU, dCnt + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    keys.resize(nU), runs.resize(nU);
    HIPCK(hipMemcpyAsync(keys.data(), kIn, (size_t)nU * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipMemcpyAsync(runs.data(), runLen, (size_t)nU * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}

// phase 2 (host): the new table -- the uploaded entries, the derived entries some sphere still uses, then the new geometry, each
// distinct bit pattern once -- and where every old entry and every key goes.  A decomposed run plans once, from the union of its
// slabs' keys and the sum of their uses, so that every slab holds the same table (migration carries component indices).
struct ResizePlan {
    std::vector<float4> table;
    std::vector<uint32_t> remap, keyIdx;
    std::vector<float> keyOldR;
    double reach = 0;  // largest |relPos| + radius of an entry in use: the extent of the largest clump after the change
};
static void resize_plan(const std::vector<float4>& hComp, uint32_t nTemplate, const std::vector<uint64_t>& keys, const std::vector<uint32_t>& runs,
                        std::vector<uint32_t> uses, ResizePlan& pl) {
    const uint32_t nC = (uint32_t)hComp.size(), nU = (uint32_t)keys.size();
    for (uint32_t u = 0; u < nU; u++)
        uses[(uint32_t)(keys[u] >> 32)] -= runs[u];
    std::map<CompBits, uint32_t> where;
    pl.table.clear();
    auto place = [&](const float4& v) {
        auto it = where.emplace(comp_bits(v), (uint32_t)pl.table.size());
        if (it.second)
            pl.table.push_back(v);
        return it.first->second;
    };
    auto reach = [&](const float4& v) {
        pl.reach = std::max(pl.reach, std::sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z) + (double)v.w);
    };
    const uint32_t nT = std::min(nTemplate, nC);
    pl.remap.assign(nC, 0), pl.keyIdx.assign(nU, 0), pl.keyOldR.assign(nU, 0.f), pl.reach = 0;
    for (uint32_t i = 0; i < nT; i++) {  // (kept whatever their bits: UpdateClumps appends clumps that refer to them by index)
        where.emplace(comp_bits(hComp[i]), i);
        pl.table.push_back(hComp[i]);
        pl.remap[i] = i;
        if (uses[i])
            reach(hComp[i]);
    }
    for (uint32_t i = nT; i < nC; i++)
        if (uses[i]) {
            pl.remap[i] = place(hComp[i]);
            reach(hComp[i]);
        }
    for (uint32_t u = 0; u < nU; u++) {
        const float4 b = hComp[(uint32_t)(keys[u] >> 32)];
        pl.keyOldR[u] = b.w;
        float f;
        const uint32_t bits = (uint32_t)keys[u];
        memcpy(&f, &bits, 4);
        const float4 v = make_float4(b.x * f, b.y * f, b.z * f, b.w * f);  // one fp32 multiply each (modifyComponents)
        pl.keyIdx[u] = place(v);
        reach(v);
    }
}

// phase 3 (device): the scratch of the apply pass first, the table last -- a failed allocation leaves the context as it was
static int resize_apply(deme_ctx* c, const std::vector<uint64_t>& keys, const ResizePlan& pl) {
    const uint32_t nS = c->nSpheres, nU = (uint32_t)keys.size();
    if (upload(c, c->rsUKeys, keys.data(), keys.size()) || upload(c, c->rsIdx, pl.keyIdx.data(), pl.keyIdx.size()) ||
        upload(c, c->rsOldR, pl.keyOldR.data(), pl.keyOldR.size()) || upload(c, c->rsRemap, pl.remap.data(), pl.remap.size()))
        return c->lastStatus;
    if (int rc = upload(c, c->comp, pl.table.data(), pl.table.size()))
        return rc;
    c->nComp = (uint32_t)pl.table.size();
    c->hComp = pl.table;
    refresh_dev_params(c);  // (the table may have moved)
    if (nS) {
        GeoRec* geo = (c->haveList && !c->geoStale && c->geo.bytes >= (size_t)nS * sizeof(GeoRec)) ? c->geo.as<GeoRec>() : nullptr;
        hipLaunchKernelGGL(k_resize_apply, dim3(grid_for(nS)), dim3(256), 0, c->stream, nS, c->spheres.as<SphereRec>(), c->dp.o2e,
                           c->rsMark.as<uint32_t>(), c->rsUKeys.as<uint64_t>(), nU, c->rsIdx.as<uint32_t>(), c->rsOldR.as<float>(),
                           c->rsRemap.as<uint32_t>(), c->comp.as<float4>(), geo);
    }
    HIPCK(hipStreamSynchronize(c->stream));
    // a critical change (the reference's announceCritical): the next step detects with the new sizes and fresh margins, the
    // history follows through the normal map; an asynchronous detection does not start from a stale list (async_detection_can_start)
    c->listStale = true;
    c->fusedPrevValid = false;
    return DEME_OK;
}

int deme_change_owner_sizes(deme_ctx* c, const uint32_t* ownerIds, const float* factors, size_t n) {
    if (int rc = check_ready(c))
        return rc;
    std::vector<uint32_t> fb;
    char msg[256];
    if (int rc = resize_check(msg, sizeof msg, ownerIds, factors, n, c->nOwners, fb))
        return fail(c, rc, "deme_change_owner_sizes: %s", msg);
    if (!n || !c->nSpheres)
        return DEME_OK;
    std::vector<uint64_t> keys;
    std::vector<uint32_t> runs, uses;
    if (int rc = resize_collect(c, ownerIds, fb.data(), n, keys, runs, uses))
        return rc;
    if (keys.empty())  // only owners without spheres (analytical objects, meshes): nothing to do, as in the reference
        return DEME_OK;
    ResizePlan pl;
    resize_plan(c->hComp, c->nTemplateComps, keys, runs, uses, pl);
    if (pl.table.size() > 65535)
        return fail(c, DEME_ERR_INVALID, "deme_change_owner_sizes: the resized scene needs %zu clump components; at most 65535 are supported "
                    "(fewer distinct factors keep the table small)", pl.table.size());
    return resize_apply(c, keys, pl);
}

int deme_set_template_components(deme_ctx* c, uint32_t n) {
    if (int rc = check_ready(c))
        return rc;
    if (n > c->nComp)
        return fail(c, DEME_ERR_INVALID, "deme_set_template_components: %u entries but the table holds %u", n, c->nComp);
    c->nTemplateComps = n;
    return DEME_OK;
}

int deme_num_components(const deme_ctx* c, uint32_t* n) {
    if (!c || !n)
        return DEME_ERR_INVALID;
    *n = c->nComp;
    return DEME_OK;
}

int deme_download_components(deme_ctx* c, float* relX, float* relY, float* relZ, float* radius, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    if (cap < c->nComp)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %u", c->nComp);
    for (uint32_t i = 0; i < c->nComp; i++) {
        const float4 v = c->hComp[i];
        if (relX) relX[i] = v.x;
        if (relY) relY[i] = v.y;
        if (relZ) relZ[i] = v.z;
        if (radius) radius[i] = v.w;
    }
    return DEME_OK;
}

int deme_download_sphere_components(deme_ctx* c, uint16_t* comp, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    const size_t n = c->nSpheres;
    if (cap < n || (n && !comp))
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", n);
    std::vector<SphereRec> h(n);
    if (n)
        HIPCK(hipMemcpyAsync(h.data(), c->spheres.p, n * sizeof(SphereRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; k++)
        comp[order_sphere_out(c, (uint32_t)k)] = h[k].comp;
    return DEME_OK;
}

// ---- contacts of a few owners (deme_query.h) ----------------------------------------------------------------------------------
// The selection runs on the engine's list as it stands; what comes to the host is the hit count and the hit rows, which are then
// put in the caller's canonical order by their caller-id keys (keys of a list are unique) -- the sub-sequence of what
// deme_download_contacts returns, without the caller's view of the whole list (order_current_view) ever being built.
// A decomposed run asks every slab the same way (deme_decomp.inc), with the slab's books: the marks are then over GLOBAL owner ids
// and the kernel applies the merged list's rules.
namespace {
// (id, row of the call) sorted by id; false when an id comes twice (*twice receives it)
inline bool owner_ids_distinct(const uint32_t* ids, size_t n, std::vector<std::pair<uint32_t, uint32_t>>& sorted, uint32_t* twice) {
    sorted.resize(n);
    for (size_t i = 0; i < n; i++)
        sorted[i] = {ids[i], (uint32_t)i};
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < n; i++)
        if (sorted[i].first == sorted[i - 1].first) {
            *twice = sorted[i].first;
            return false;
        }
    return true;
}
// The refusals the by-owner entry points share, in the order they make them; DEME_OK, or the code with the text in msg for the
// caller's fail / mfail.  `who`: the entry point; `other` (named otherName): its second pointer; st with accWhy: a state whose a /
// alpha columns are refused; count32: ids are counted in 32 bits; sorted: filled by owner_ids_distinct, an id given twice refused.
int owner_ids_refused(char (&msg)[320], const char* who, const void* other, const char* otherName, const uint32_t* ids, size_t n, uint32_t nOwners,
                      const DemeOwnerState* st = nullptr, const char* accWhy = nullptr, bool count32 = false,
                      std::vector<std::pair<uint32_t, uint32_t>>* sorted = nullptr) {
    uint32_t twice = 0;
    if (!other || (n && !ids))
        snprintf(msg, sizeof msg, "%s: null %s", who, other ? "owner id array" : otherName);
    else if (st && owner_state_wants_acc(st))
        snprintf(msg, sizeof msg, "%s: a / alpha %s", who, accWhy);
    else if (count32 && n > 0xFFFFFFFFull)
        snprintf(msg, sizeof msg, "%s: %zu ids", who, n);
    else if (const uint32_t* bad = std::find_if(ids, ids + n, [&](uint32_t id) { return id >= nOwners; }); bad != ids + n)
        snprintf(msg, sizeof msg, "%s: owner id %u is out of range (%u owners)", who, *bad, nOwners);
    else if (sorted && !owner_ids_distinct(ids, n, *sorted, &twice))
        snprintf(msg, sizeof msg, "%s: owner id %u is given twice (the order of two writes is not defined)", who, twice);
    else
        return DEME_OK;
    return DEME_ERR_INVALID;
}
// the distinct ids of a question, marked in the context's byte array of nMarks entries
int query_mark(deme_ctx* c, const std::vector<uint32_t>& ids, size_t nMarks) {
    if (ensure(c, c->qMark, nMarks) || ensure(c, c->qCtr, 256) || ensure(c, c->stage, std::max<size_t>(ids.size(), 1) * 4))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->qMark.p, 0, nMarks, c->stream));
    if (!ids.empty()) {
        HIPCK(hipMemcpyAsync(c->stage.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_query_mark, dim3(grid_for(ids.size())), dim3(256), 0, c->stream, (uint32_t)ids.size(), c->stage.as<uint32_t>(),
                           c->qMark.as<uint8_t>());
    }
    return DEME_OK;
}
// the tables a row's owners are looked up in (row_owners); s2e and o2e stay null: the inspectors work in owner slots
QueryTables query_tables(const deme_ctx* c) {
    QueryTables t{};
    t.spheres = c->spheres.as<SphereRec>(), t.tris = c->tris.as<TriRec>(), t.anal = c->anal.as<AnalObj>();
    t.nSpheres = c->nSpheres, t.nTri = c->nTri, t.nAnal = c->nAnal, t.nOwners = c->nOwners;
    return t;
}
// The force threshold of the inspectors: what every one of them refuses of it (the text goes to msg), and the square the kernels
// compare with (row_force_counted).
bool threshold_refused(char (&msg)[320], const char* who, float thr) {
    if (std::isfinite(thr) && thr >= 0.f)
        return false;
    snprintf(msg, sizeof msg, "%s: the force threshold is %g; it must be finite and >= 0", who, (double)thr);
    return true;
}
inline double threshold_sq(float thr) { return (double)thr * (double)thr; }
// one context's selection: the hit count in nHit, the hits (and records) left in the context's scratch; passes: count read-backs
// made.  bk: the books of a slab, null for a single context; who: the entry point, for the message.
int query_select(deme_ctx* c, const SlabBooksDev* bk, const char* who, int withRecords, uint32_t& nHit, uint32_t& passes) {
    nHit = 0, passes = 0;
    const size_t n = c->haveList ? (size_t)c->nContacts : 0;
    if (!n)
        return DEME_OK;
    QueryTables t = query_tables(c);
    t.s2e = c->dp.s2e, t.o2e = c->dp.o2e;
    size_t want = 256;  // rows of scratch a first query starts with
    for (int pass = 0;; pass++) {
        if (ensure(c, c->qHits, want * sizeof(QueryHit)) || (withRecords && ensure(c, c->qRecs, want * 48)))
            return c->lastStatus;
        size_t rows = c->qHits.bytes / sizeof(QueryHit);  // the kernel's bound is what the allocations hold, whatever was asked for
        if (withRecords)
            rows = std::min(rows, c->qRecs.bytes / 48);
        rows = std::min<size_t>(rows, 0xFFFFFFFFu);
        HIPCK(hipMemsetAsync(c->qCtr.p, 0, 4, c->stream));
        hipLaunchKernelGGL(bk ? k_query_select<true> : k_query_select<false>, dim3(grid_for(n)), dim3(256), 0, c->stream, (uint32_t)n,
                           c->keysSorted[c->keysCur].as<uint64_t>(), t, bk ? *bk : SlabBooksDev{}, c->qMark.as<uint8_t>(),
                           withRecords ? c->rec[0].as<float>() : nullptr, withRecords ? c->rec[1].as<float>() : nullptr,
                           withRecords ? c->rec[2].as<float>() : nullptr, withRecords ? c->rec[3].as<float>() : nullptr,
                           c->qHits.as<QueryHit>(), withRecords ? c->qRecs.as<float>() : nullptr, (uint32_t)rows, c->qCtr.as<uint32_t>());
        HIPCK(hipMemcpyAsync(&nHit, c->qCtr.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipStreamSynchronize(c->stream));
        passes++;
        if (nHit <= rows)
            return DEME_OK;
        if (pass)  // (the list cannot change between two selections)
            return fail(c, DEME_ERR_OVERFLOW, "%s: %u hits after the scratch was sized for them", who, nHit);
        want = nHit;
    }
}
int query_fetch(deme_ctx* c, uint32_t nHit, int withRecords, QueryHit* h, float* r) {
    HIPCK(hipMemcpyAsync(h, c->qHits.p, (size_t)nHit * sizeof(QueryHit), hipMemcpyDeviceToHost, c->stream));
    if (withRecords)
        HIPCK(hipMemcpyAsync(r, c->qRecs.p, (size_t)nHit * 48, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
// what an owner-contact query hands back, row by row; a null column is not asked
struct QueryRows {
    uint32_t *idA, *idB;
    uint8_t* type;
    uint32_t *ownerA, *ownerB;
    uint8_t* side;
    float* rec[4];  // force, torque-only force, cpA, cpB
};
// The fetched hits in the order of their keys (keys of a list are unique).  merged: the keys are merged_key's, not the caller's
// contact keys; ctxOf(hit): the context whose hObjType answers for an analytical row.
template <class CtxOf>
void query_emit(const std::vector<QueryHit>& h, const std::vector<float>& r, bool merged, CtxOf ctxOf, const QueryRows& out) {
    std::vector<uint32_t> perm(h.size());
    for (size_t i = 0; i < perm.size(); i++)
        perm[i] = (uint32_t)i;
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return h[a].key < h[b].key; });
    for (size_t i = 0; i < perm.size(); i++) {
        const QueryHit& q = h[perm[i]];
        const uint32_t cls = key_class(q.key), a = merged ? merged_key_a(q.key) : key_a(q.key), b = merged ? merged_key_b(q.key) : key_b(q.key);
        if (out.idA)
            out.idA[i] = a;
        if (out.idB)
            out.idB[i] = b;
        if (out.type)
            out.type[i] = cls == DEME_KEY_CLASS_SS   ? DEME_SPHERE_SPHERE_CONTACT
                          : cls == DEME_KEY_CLASS_SM ? DEME_SPHERE_MESH_CONTACT
                          : ctxOf(perm[i])->hObjType[b] == DEME_ANAL_OBJ_TYPE_PLANE ? DEME_SPHERE_PLANE_CONTACT
                                                                                    : DEME_SPHERE_CYL_CONTACT;
        if (out.ownerA)
            out.ownerA[i] = q.ownerA;
        if (out.ownerB)
            out.ownerB[i] = q.ownerB;
        if (out.side)
            out.side[i] = (uint8_t)(q.side & 1u);  // (bit 1, DEME_QUERY_FLIPPED, is a slab's own business)
        if (!r.empty())
            for (int k = 0; k < 4; k++)
                if (out.rec[k])
                    memcpy(out.rec[k] + 3 * i, r.data() + 12 * (size_t)perm[i] + 3 * k, 12);
    }
}
}  // namespace

int deme_query_owner_contacts(deme_ctx* c, const uint32_t* ownerIds, size_t nOwners, int withRecords, uint32_t* idA, uint32_t* idB,
                              uint8_t* type, uint32_t* ownerA, uint32_t* ownerB, uint8_t* side, float* force, float* torqueOnly,
                              float* cpA, float* cpB, size_t cap, size_t* nOut) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = owner_ids_refused(msg, "deme_query_owner_contacts", nOut, "nOut", ownerIds, nOwners, c->nOwners))
        return fail(c, rc, "%s", msg);
    if (withRecords)
        if (int rc = records_refused(c))
            return rc;
    std::vector<uint32_t> ids(ownerIds, ownerIds + nOwners);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    uint32_t nHit = 0, passes = 0;
    if (c->haveList && c->nContacts && !ids.empty()) {  // (a context with an empty list, or an empty question, is not asked)
        if (int rc = query_mark(c, ids, c->nOwners))
            return rc;
        const int rc = query_select(c, nullptr, "deme_query_owner_contacts", withRecords, nHit, passes);
        c->qHostBytes += 4ull * passes;
        if (rc)
            return rc;
    }
    *nOut = nHit;
    if (cap < nHit)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", (size_t)nHit);
    if (!nHit)
        return DEME_OK;
    std::vector<QueryHit> h(nHit);
    std::vector<float> r(withRecords ? (size_t)nHit * 12 : 0);
    if (int rc = query_fetch(c, nHit, withRecords, h.data(), r.data()))
        return rc;
    c->qHostBytes += (uint64_t)nHit * (sizeof(QueryHit) + (withRecords ? 48 : 0));
    query_emit(h, r, false, [&](uint32_t) { return c; }, QueryRows{idA, idB, type, ownerA, ownerB, side, {force, torqueOnly, cpA, cpB}});
    return DEME_OK;
}

int deme_query_host_bytes(const deme_ctx* c, uint64_t* bytes) {
    if (!c || !bytes)
        return DEME_ERR_INVALID;
    *bytes = c->qHostBytes;
    return DEME_OK;
}

// ---- contact inspectors: virial sum and counted sides of the current list (deme_contact_inspect.h) ----------------------------------
namespace {
// the refusals deme_inspect_contacts and deme_inspect_contact_counts share, in the order they make them (the last are those of
// deme_download_contact_records: records_refused)
int contact_inspect_refused(deme_ctx* c, const char* who, const void* out, int region, float thr) {
    if (!out)
        return fail(c, DEME_ERR_INVALID, "%s: null output", who);
    if (region < -1 || region >= (int)c->regionFn.size())
        return fail(c, DEME_ERR_INVALID, "unknown inspection region %d", region);
    char msg[320];
    if (threshold_refused(msg, who, thr))
        return fail(c, DEME_ERR_INVALID, "%s", msg);
    if (int rc = records_refused(c))
        return rc;
    return DEME_OK;
}
// The passes of one context, enqueued on its stream.  perOwner false: the result is left in ciPartial behind the blocks' partials
// (*res points at it).  perOwner true: the counted sides per owner SLOT are left in ciCounts.  Nothing the step reads is written.
int contact_inspect_launch(deme_ctx* c, int region, float thr, bool perOwner, ContactSums** res) {
    const size_t n = c->haveList ? (size_t)c->nContacts : 0, nO = c->nOwners;
    const unsigned grid = grid_for(std::max<size_t>(std::max(n, nO), 1));
    if (ensure(c, c->ciMask, std::max<size_t>(nO, 1) * 4) || ensure(c, c->ciPartial, ((size_t)grid + 1) * sizeof(ContactSums)) ||
        (perOwner && ensure(c, c->ciCounts, std::max<size_t>(nO, 1) * 4)))
        return c->lastStatus;
    if (nO) {
        hipLaunchKernelGGL(k_contact_owner_mask, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, c->owners.as<OwnerRec>(),
                           (uint32_t)c->nOwnerClumps, c->dp.o2e, c->ciMask.as<float>());
        if (region >= 0) {  // the owners' centres of mass, as deme_inspect_region tests them
            DevParams dp = c->dp;
            const OwnerRec* owners = c->owners.as<OwnerRec>();
            const SphereRec* spheres = c->spheres.as<SphereRec>();
            uint32_t nn = (uint32_t)nO, ps = 0u;
            float identity = 0.f;
            float* values = c->ciMask.as<float>();
            void* args[] = {&dp, &owners, &spheres, &nn, &ps, &identity, &values};
            HIPCK(hipModuleLaunchKernel(c->regionFn[region], grid_for(nO), 1, 1, 256, 1, 1, 0, c->stream, args, nullptr));
        }
    }
    ContactSumArgs a{};
    a.n = (uint32_t)n, a.nSlots = (uint32_t)nO, a.keys = c->keysSorted[c->keysCur].as<uint64_t>();
    a.t = query_tables(c), a.owners = c->owners.as<OwnerRec>(), a.mask = c->ciMask.as<float>();
    a.force = c->rec[0].as<float>(), a.cpA = c->rec[2].as<float>(), a.cpB = c->rec[3].as<float>();
    a.thr2 = threshold_sq(thr);
    a.partial = c->ciPartial.as<ContactSums>(), a.counts = c->ciCounts.as<uint32_t>();
    if (perOwner) {
        HIPCK(hipMemsetAsync(c->ciCounts.p, 0, std::max<size_t>(nO, 1) * 4, c->stream));
        if (n)
            hipLaunchKernelGGL(k_contact_sums<true>, dim3(grid_for(n)), dim3(256), 0, c->stream, a);
        return DEME_OK;
    }
    hipLaunchKernelGGL(k_contact_sums<false>, dim3(grid), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_contact_sums_final, dim3(1), dim3(256), 0, c->stream, (uint32_t)grid, a.partial, a.partial + grid);
    *res = a.partial + grid;
    return DEME_OK;
}
}  // namespace

int deme_inspect_contacts(deme_ctx* c, int region, float thr, DemeContactSums* out) {
    static_assert(sizeof(DemeContactSums) == sizeof(ContactSums), "DemeContactSums is the device's ContactSums");
    if (int rc = check_ready(c))
        return rc;
    if (int rc = contact_inspect_refused(c, "deme_inspect_contacts", out, region, thr))
        return rc;
    ContactSums* res = nullptr;
    if (int rc = contact_inspect_launch(c, region, thr, false, &res))
        return rc;
    DemeContactSums h;
    HIPCK(hipMemcpyAsync(&h, res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->qHostBytes += sizeof h;
    *out = h;
    return DEME_OK;
}

int deme_inspect_contact_counts(deme_ctx* c, int region, float thr, uint32_t* perOwner, size_t cap) {
    if (int rc = check_ready(c))
        return rc;
    if (int rc = contact_inspect_refused(c, "deme_inspect_contact_counts", perOwner, region, thr))
        return rc;
    const size_t nO = c->nOwners;
    if (cap < nO)
        return fail(c, DEME_ERR_INVALID, "buffer too small: need %zu", nO);
    if (!nO)
        return DEME_OK;
    if (ensure(c, c->ciOut, nO * 4))
        return c->lastStatus;
    if (int rc = contact_inspect_launch(c, region, thr, true, nullptr))
        return rc;
    if (nO)  // (an ownerless scene: no launch of no workgroups, see deme_set_margins)
    hipLaunchKernelGGL(k_contact_counts_out, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, c->ciCounts.as<uint32_t>(), c->dp.o2e,
                       (const uint32_t*)nullptr, c->ciOut.as<uint32_t>(), (uint32_t)nO);
    std::vector<uint32_t> h(nO);
    HIPCK(hipMemcpyAsync(h.data(), c->ciOut.p, nO * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->qHostBytes += 4ull * nO;
    memcpy(perOwner, h.data(), nO * 4);
    return DEME_OK;
}

// ---- contact loads per mesh triangle (deme_tri_loads.h) -----------------------------------------------------------------------------
namespace {
// what deme_inspect_tri_loads refuses of its arguments, in the order it does (c null: a decomposed run asking before any slab is;
// the text goes to msg)
int tri_loads_args_refused(char (&msg)[320], const char* who, float thr, uint32_t firstTri, uint32_t nTris, uint32_t nTri, const void* force,
                           const void* contacts) {
    msg[0] = 0;
    if (threshold_refused(msg, who, thr))
        return DEME_ERR_INVALID;
    if ((uint64_t)firstTri + nTris > nTri)
        snprintf(msg, sizeof msg, "%s: triangles [%u, %llu) were asked for; the scene has %u", who, firstTri,
                 (unsigned long long)firstTri + nTris, nTri);
    else if (nTris && !force && !contacts)
        snprintf(msg, sizeof msg, "%s: null output (force and contacts)", who);
    return msg[0] ? DEME_ERR_INVALID : DEME_OK;
}
// The passes of one context, enqueued on its stream: the sums of every triangle are left in tlForce (3 doubles a triangle) and
// tlCount.  Nothing the step reads is written.
int tri_loads_launch(deme_ctx* c, float thr) {
    const size_t n = c->haveList ? (size_t)c->nContacts : 0, nT = c->nTri;
    if (ensure(c, c->tlForce, nT * 24) || ensure(c, c->tlCount, nT * 4))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->tlForce.p, 0, nT * 24, c->stream));
    HIPCK(hipMemsetAsync(c->tlCount.p, 0, nT * 4, c->stream));
    if (!n)
        return DEME_OK;
    if (int rc = seg_reserve(c, c->tlPairs, n))
        return rc;
    TriSelectArgs a{};
    a.n = (uint32_t)n, a.keys = c->keysSorted[c->keysCur].as<uint64_t>();
    a.spheres = c->spheres.as<SphereRec>(), a.owners = c->owners.as<OwnerRec>();
    a.nSpheres = c->nSpheres, a.nOwners = c->nOwners, a.nTri = c->nTri;
    a.force = c->rec[0].as<float>(), a.thr2 = threshold_sq(thr);
    a.tri = c->tlPairs.key[0].as<uint32_t>(), a.row = c->tlPairs.val[0].as<uint32_t>();
    {
        ScopedTimer t(c, "tri_loads_select", true);
        hipLaunchKernelGGL(k_tri_select, dim3(grid_for(n)), dim3(256), 0, c->stream, a);
    }
    {
        ScopedTimer t(c, "tri_loads_sort", true);
        if (int rc = seg_sort(c, c->tlPairs, n, nT))
            return rc;
    }
    ScopedTimer t(c, "tri_loads_sums", true);
    if (int rc = seg_sums<TRI_LANES>(c, c->tlPairs, n, nT, TriTerm{c->tlPairs.val[1].as<uint32_t>(), c->rec[0].as<float>()},
                                     TriOut{c->tlForce.as<double>(), c->tlCount.as<uint32_t>()}))
        return rc;
    HIPCK(hipGetLastError());
    return DEME_OK;
}
// the asked range of the sums tri_loads_launch left, to host arrays (either may be null); waits for the stream
int tri_loads_fetch(deme_ctx* c, uint32_t firstTri, uint32_t nTris, double* force, uint32_t* contacts) {
    if (force)
        HIPCK(hipMemcpyAsync(force, c->tlForce.as<double>() + 3 * (size_t)firstTri, (size_t)nTris * 24, hipMemcpyDeviceToHost, c->stream));
    if (contacts)
        HIPCK(hipMemcpyAsync(contacts, c->tlCount.as<uint32_t>() + firstTri, (size_t)nTris * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

unsigned deme_tri_loads_block_rows(void) { return SEG_BLOCK_ROWS; }

int deme_inspect_tri_loads(deme_ctx* c, float thr, uint32_t firstTri, uint32_t nTris, double* force, uint32_t* contacts) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = tri_loads_args_refused(msg, "deme_inspect_tri_loads", thr, firstTri, nTris, c->nTri, force, contacts))
        return fail(c, rc, "%s", msg);
    if (!nTris)
        return DEME_OK;
    if (records_refused(c))
        return fail(c, DEME_ERR_INVALID, "deme_inspect_tri_loads: %s", std::string(c->err).c_str());
    if (int rc = tri_loads_launch(c, thr))
        return rc;
    std::vector<double> hf(force ? (size_t)nTris * 3 : 0);  // (the caller's arrays are written once the call cannot fail any more)
    std::vector<uint32_t> hn(contacts ? nTris : 0);
    if (int rc = tri_loads_fetch(c, firstTri, nTris, force ? hf.data() : nullptr, contacts ? hn.data() : nullptr))
        return rc;
    c->qHostBytes += (uint64_t)nTris * ((force ? 24 : 0) + (contacts ? 4 : 0));
    if (force)
        memcpy(force, hf.data(), hf.size() * 8);
    if (contacts)
        memcpy(contacts, hn.data(), hn.size() * 4);
    return DEME_OK;
}

// ---- mesh wear: impulse and sliding work per triangle, summed over the samples of a run (deme_tri_wear.h) -----------------------------
namespace {
// the accumulators of nTri triangles, cleared (enqueued; the context keeps them until the feature is disabled)
int tri_wear_clear(deme_ctx* c) {
    const size_t nT = c->nTri;
    if (ensure(c, c->twAcc, nT * WEAR_LANES * 8) || ensure(c, c->twRows, nT * 8))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->twAcc.p, 0, std::max<size_t>(nT * WEAR_LANES * 8, 1), c->stream));
    HIPCK(hipMemsetAsync(c->twRows.p, 0, std::max<size_t>(nT * 8, 1), c->stream));
    c->twTri = c->nTri, c->twTime = 0;
    return DEME_OK;
}
// what deme_tri_wear_sample refuses before it looks at the list, in the order it does (the text goes to msg)
int tri_wear_sample_refused(char (&msg)[320], const char* who, bool enabled, float thr, double weight) {
    msg[0] = 0;
    if (!enabled)
        snprintf(msg, sizeof msg, "%s: mesh wear accumulation is not enabled (deme_tri_wear_enable)", who);
    else if (threshold_refused(msg, who, thr))
        ;
    else if (!(std::isfinite(weight) && weight >= 0.0))
        snprintf(msg, sizeof msg, "%s: the weight is %g; it must be finite and >= 0", who, weight);
    return msg[0] ? DEME_ERR_INVALID : DEME_OK;
}
// A list the force pass has not evaluated: a seed, or one that was just put in force -- by deme_detect_contacts, or by an
// asynchronous detection whose cycle ended with the call -- so that the records in memory are those of the list before it and say
// nothing of its rows.  (conValid: the contributions in memory are those of the list in force.)
inline bool tri_wear_list_unevaluated(const deme_ctx* c) { return c->haveList && (c->seeded || !c->conValid); }
// The passes of one sample of one context, enqueued on its stream behind the steps already there; no read-back, no wait.  n is the
// host's count of the list; the key nTri of the rows that do not count does the compaction (deme_tri_loads.h).  Nothing the step
// reads is written.
int tri_wear_launch(deme_ctx* c, float thr, double weight) {
    const size_t n = c->haveList ? (size_t)c->nContacts : 0, nT = c->nTri;
    c->twTime += weight;
    if (!n || !nT)
        return DEME_OK;
    if (int rc = seg_reserve(c, c->tlPairs, n))
        return rc;
    TriSelectArgs a{};
    a.n = (uint32_t)n, a.keys = c->keysSorted[c->keysCur].as<uint64_t>();
    a.spheres = c->spheres.as<SphereRec>(), a.owners = c->owners.as<OwnerRec>();
    a.nSpheres = c->nSpheres, a.nOwners = c->nOwners, a.nTri = c->nTri;
    a.force = c->rec[0].as<float>(), a.thr2 = threshold_sq(thr);
    a.tri = c->tlPairs.key[0].as<uint32_t>(), a.row = c->tlPairs.val[0].as<uint32_t>();
    {
        ScopedTimer t(c, "tri_wear_select", true);
        hipLaunchKernelGGL(k_tri_select, dim3(grid_for(n)), dim3(256), 0, c->stream, a);
    }
    {
        ScopedTimer t(c, "tri_wear_sort", true);
        if (int rc = seg_sort(c, c->tlPairs, n, nT))
            return rc;
    }
    ScopedTimer t(c, "tri_wear_sums", true);
    const WearTerm term{c->tlPairs.val[1].as<uint32_t>(), (uint32_t)n, a.keys, query_tables(c), a.owners, c->rec[0].as<float>(),
                        c->rec[2].as<float>(), c->rec[3].as<float>(), weight};
    if (int rc = seg_sums<WEAR_LANES>(c, c->tlPairs, n, nT, term, WearOut{c->twAcc.as<double>(), c->twRows.as<uint64_t>()}))
        return rc;
    HIPCK(hipGetLastError());
    return DEME_OK;
}
// what deme_tri_wear_read refuses of its arguments, in the order it does (the text goes to msg)
int tri_wear_read_refused(char (&msg)[320], const char* who, bool enabled, uint32_t firstTri, uint32_t nTris, uint32_t nTri, bool anyOutput) {
    msg[0] = 0;
    if (!enabled)
        snprintf(msg, sizeof msg, "%s: mesh wear accumulation is not enabled (deme_tri_wear_enable)", who);
    else if ((uint64_t)firstTri + nTris > nTri)
        snprintf(msg, sizeof msg, "%s: triangles [%u, %llu) were asked for; the scene has %u", who, firstTri,
                 (unsigned long long)firstTri + nTris, nTri);
    else if (nTris && !anyOutput)
        snprintf(msg, sizeof msg, "%s: null output (every column and sampledTime)", who);
    return msg[0] ? DEME_ERR_INVALID : DEME_OK;
}
// The columns of deme_tri_wear_read in its order -- impulse, normalImpulse, slidingWork, shearWork, rows -- and their bytes a triangle
constexpr size_t WEAR_COL_BYTES[5] = {24, 8, 8, 8, 8};
inline size_t tri_wear_bytes(uint32_t nTris, const bool (&want)[5]) {
    size_t b = 0;
    for (int j = 0; j < 5; j++)
        b += want[j] ? WEAR_COL_BYTES[j] * nTris : 0;
    return b;
}
// The asked columns of the asked range, packed one behind the other on the device (k_tri_wear_gather) and copied to h in one piece:
// tri_wear_bytes of them, no more.  Waits for the stream.
int tri_wear_fetch(deme_ctx* c, uint32_t firstTri, uint32_t nTris, const bool (&want)[5], std::vector<char>& h) {
    const size_t bytes = tri_wear_bytes(nTris, want);
    h.resize(bytes);
    if (!bytes)
        return DEME_OK;
    if (int rc = ensure(c, c->twOut, bytes))
        return rc;
    char* at[5];
    size_t off = 0;
    for (int j = 0; j < 5; j++) {
        at[j] = want[j] ? (char*)c->twOut.p + off : nullptr;
        off += want[j] ? WEAR_COL_BYTES[j] * nTris : 0;
    }
    const WearGatherArgs a{firstTri, nTris, c->twAcc.as<double>(), c->twRows.as<uint64_t>(), (double*)at[0], (double*)at[1], (double*)at[2],
                           (double*)at[3], (uint64_t*)at[4]};
    hipLaunchKernelGGL(k_tri_wear_gather, dim3(grid_for(nTris)), dim3(256), 0, c->stream, a);
    HIPCK(hipMemcpyAsync(h.data(), c->twOut.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
// column j of a fetched block
inline const char* tri_wear_column(const std::vector<char>& h, uint32_t nTris, const bool (&want)[5], int j) {
    size_t off = 0;
    for (int k = 0; k < j; k++)
        off += want[k] ? WEAR_COL_BYTES[k] * nTris : 0;
    return h.data() + off;
}
}  // namespace

int deme_tri_wear_enable(deme_ctx* c, int on) {
    if (int rc = check_ready(c))
        return rc;
    if (!on) {
        if (c->twOn)
            HIPCK(hipStreamSynchronize(c->stream));  // (a sample may still be adding)
        for (DevBuf* b : {&c->twAcc, &c->twRows, &c->twOut})
            if (b->p) {
                HIPCK(hipFree(b->p));
                *b = DevBuf{};
            }
        c->twOn = false, c->twTri = 0, c->twTime = 0;
        return DEME_OK;
    }
    if (c->twOn)
        return DEME_OK;  // (the sums stay)
    if (int rc = tri_wear_clear(c))
        return rc;
    c->twOn = true;
    return DEME_OK;
}

int deme_tri_wear_reset(deme_ctx* c) {
    if (int rc = check_ready(c))
        return rc;
    if (!c->twOn)
        return fail(c, DEME_ERR_INVALID, "deme_tri_wear_reset: mesh wear accumulation is not enabled (deme_tri_wear_enable)");
    return tri_wear_clear(c);
}

int deme_tri_wear_sample(deme_ctx* c, float thr, double weight, int* sampled) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = tri_wear_sample_refused(msg, "deme_tri_wear_sample", c->twOn, thr, weight))
        return fail(c, rc, "%s", msg);
    if (!c->record)
        return fail(c, DEME_ERR_INVALID, "deme_tri_wear_sample: contact recording is off (deme_set_record_contacts)");
    if (sampled)
        *sampled = 0;
    if (tri_wear_list_unevaluated(c))  // the caller carries the weight to its next sample
        return DEME_OK;
    if (int rc = tri_wear_launch(c, thr, weight))
        return rc;
    if (sampled)
        *sampled = 1;
    return DEME_OK;
}

int deme_tri_wear_read(deme_ctx* c, uint32_t firstTri, uint32_t nTris, double* impulse, double* normalImpulse, double* slidingWork,
                       double* shearWork, uint64_t* rows, double* sampledTime) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    const bool any = impulse || normalImpulse || slidingWork || shearWork || rows || sampledTime;
    if (int rc = tri_wear_read_refused(msg, "deme_tri_wear_read", c->twOn, firstTri, nTris, c->nTri, any))
        return fail(c, rc, "%s", msg);
    if (nTris) {
        void* dst[5] = {impulse, normalImpulse, slidingWork, shearWork, rows};
        const bool want[5] = {impulse != nullptr, normalImpulse != nullptr, slidingWork != nullptr, shearWork != nullptr, rows != nullptr};
        std::vector<char> h;  // (the caller's arrays are written once the call cannot fail any more)
        if (int rc = tri_wear_fetch(c, firstTri, nTris, want, h))
            return rc;
        c->qHostBytes += h.size();
        for (int j = 0; j < 5; j++)
            if (want[j])
                memcpy(dst[j], tri_wear_column(h, nTris, want, j), WEAR_COL_BYTES[j] * nTris);
    }
    if (sampledTime)
        *sampledTime = c->twTime;
    return DEME_OK;
}

// ---- per-cell sums on a grid (deme_fields.h) ------------------------------------------------------------------------------------------
namespace {
constexpr size_t FIELD_CELL_BYTES = 168;  // of fiOut: two counts and 20 doubles a cell
// what deme_inspect_fields refuses of its arguments alone, in the order it does (the text goes to msg)
int fields_args_refused(char (&msg)[320], const char* who, const DemeFieldGrid* g, float thr, const DemeFieldColumns* out) {
    msg[0] = 0;
    if (!g || !out) {
        snprintf(msg, sizeof msg, "%s: null %s", who, !g ? "grid" : "columns");
        return DEME_ERR_INVALID;
    }
    bool finite = true, positive = true, cells = true;
    for (int k = 0; k < 3; k++)
        finite = finite && std::isfinite(g->origin[k]) && std::isfinite(g->cell[k]), positive = positive && g->cell[k] > 0.0, cells = cells && g->n[k];
    const uint64_t cap = DEME_FIELDS_MAX_CELLS;
    if (!finite)
        snprintf(msg, sizeof msg, "%s: the grid's origin (%g, %g, %g) and cell edges (%g, %g, %g) must be finite", who, g->origin[0], g->origin[1],
                 g->origin[2], g->cell[0], g->cell[1], g->cell[2]);
    else if (!positive)
        snprintf(msg, sizeof msg, "%s: the cell edges are (%g, %g, %g); each must be > 0", who, g->cell[0], g->cell[1], g->cell[2]);
    else if (!cells)
        snprintf(msg, sizeof msg, "%s: the grid has %u x %u x %u cells; each count must be > 0", who, g->n[0], g->n[1], g->n[2]);
    else if (g->n[0] > cap || (uint64_t)g->n[0] * g->n[1] > cap || (uint64_t)g->n[0] * g->n[1] * g->n[2] > cap)  // (no product overflows)
        snprintf(msg, sizeof msg, "%s: the grid has %u x %u x %u cells; at most %llu in all", who, g->n[0], g->n[1], g->n[2], (unsigned long long)cap);
    else if (!out->clumps && !out->mass && !out->volume && !out->momentum && !out->kinetic && !out->sides && !out->virial)
        snprintf(msg, sizeof msg, "%s: null output (every column)", who);
    else
        threshold_refused(msg, who, thr);
    return msg[0] ? DEME_ERR_INVALID : DEME_OK;
}
inline bool fields_ask_owner(const DemeFieldColumns* o) { return o->clumps || o->mass || o->volume || o->momentum || o->kinetic; }
inline bool fields_ask_contact(const DemeFieldColumns* o) { return o->sides || o->virial; }
// what one context refuses of a question whose arguments are in order (the text is left in c->err)
int fields_ctx_refused(deme_ctx* c, const DemeFieldColumns* out) {
    if (out->volume && !c->haveVolumes)
        return fail(c, DEME_ERR_INVALID, "clump_volume needs the templates' volumes (deme_upload_volumes)");
    if (!fields_ask_contact(out))
        return DEME_OK;
    if (int rc = records_refused(c))
        return rc;
    if (c->haveList && c->nContacts >= ((uint64_t)1 << 31))
        return fail(c, DEME_ERR_INVALID, "the list has %llu rows; two entries a row are indexed with 32 bits", (unsigned long long)c->nContacts);
    return DEME_OK;
}
// the columns of nC cells in fiOut
struct FieldOutDev {
    FieldOwnerOut own;
    FieldSideOut side;
};
FieldOutDev fields_out(deme_ctx* c, size_t nC) {
    char* b = c->fiOut.as<char>();
    double* d = reinterpret_cast<double*>(b + 8 * nC);
    FieldOutDev o;
    o.own.clumps = reinterpret_cast<uint32_t*>(b), o.side.sides = reinterpret_cast<uint32_t*>(b) + nC;
    o.own.mass = d, o.own.volume = d + nC, o.own.momentum = d + 2 * nC, o.own.kinetic = d + 5 * nC, o.side.virial = d + 11 * nC;
    return o;
}
// The passes of one context, enqueued on its stream: the asked groups of columns are left in fiOut.  Nothing the step reads is
// written.
int fields_launch(deme_ctx* c, const DemeFieldGrid* g, float thr, bool askOwner, bool askContact) {
    const size_t nO = c->nOwners, n = askContact && c->haveList ? (size_t)c->nContacts : 0;
    const size_t nC = (size_t)g->n[0] * g->n[1] * g->n[2];
    if (ensure(c, c->fiOut, nC * FIELD_CELL_BYTES))
        return c->lastStatus;
    const FieldOutDev o = fields_out(c, nC);
    if (askOwner) {
        HIPCK(hipMemsetAsync(o.own.clumps, 0, nC * 4, c->stream));
        HIPCK(hipMemsetAsync(o.own.mass, 0, nC * 11 * 8, c->stream));
    }
    if (askContact) {
        HIPCK(hipMemsetAsync(o.side.sides, 0, nC * 4, c->stream));
        HIPCK(hipMemsetAsync(o.side.virial, 0, nC * 9 * 8, c->stream));
    }
    if (!nO)
        return DEME_OK;
    if (ensure(c, c->fiCellOf, nO * 4) || seg_reserve(c, c->fiOwn, nO) || (n && seg_reserve(c, c->fiSide, 2 * n)))
        return c->lastStatus;
    const QueryTables t = query_tables(c);
    {
        ScopedTimer tm(c, "fields_cells", true);
        FieldCellArgs a{};
        a.nSlots = (uint32_t)nO, a.nClumps = c->nOwnerClumps, a.nCells = (uint32_t)nC, a.owners = c->owners.as<OwnerRec>();
        for (int k = 0; k < 3; k++)
            a.g.origin[k] = g->origin[k], a.g.cell[k] = g->cell[k], a.g.n[k] = g->n[k];
        a.cellOf = c->fiCellOf.as<uint32_t>(), a.key = c->fiOwn.key[0].as<uint32_t>(), a.slot = c->fiOwn.val[0].as<uint32_t>();
        hipLaunchKernelGGL(k_field_cells, dim3(grid_for(nO)), dim3(256), 0, c->stream, c->dp, a);
        if (n) {
            FieldSideSelectArgs s{};
            s.n = (uint32_t)n, s.nSlots = (uint32_t)nO, s.nCells = (uint32_t)nC, s.keys = c->keysSorted[c->keysCur].as<uint64_t>(), s.t = t;
            s.cellOf = c->fiCellOf.as<uint32_t>(), s.force = c->rec[0].as<float>(), s.thr2 = threshold_sq(thr);
            s.key = c->fiSide.key[0].as<uint32_t>(), s.val = c->fiSide.val[0].as<uint32_t>();
            hipLaunchKernelGGL(k_field_side_select, dim3(grid_for(n)), dim3(256), 0, c->stream, s);
        }
    }
    {
        ScopedTimer tm(c, "fields_sort", true);
        if (askOwner)
            if (int rc = seg_sort(c, c->fiOwn, nO, nC))
                return rc;
        if (n)
            if (int rc = seg_sort(c, c->fiSide, 2 * n, nC))
                return rc;
    }
    ScopedTimer tm(c, "fields_sums", true);
    if (askOwner) {
        const FieldOwnerTerm term{c->fiOwn.val[1].as<uint32_t>(), c->owners.as<OwnerRec>(), c->massProps.as<float4>(),
                                  c->haveVolumes ? c->volumes.as<float>() : (const float*)nullptr};
        if (int rc = seg_sums<FIELD_OWNER_LANES>(c, c->fiOwn, nO, nC, term, o.own))
            return rc;
    }
    FieldSideTerm side{};  // (no launch for an empty list: seg_sums)
    side.nSlots = (uint32_t)nO, side.vals = c->fiSide.val[1].as<uint32_t>(), side.list = c->keysSorted[c->keysCur].as<uint64_t>();
    side.t = t, side.owners = c->owners.as<OwnerRec>();
    side.force = c->rec[0].as<float>(), side.cpA = c->rec[2].as<float>(), side.cpB = c->rec[3].as<float>();
    if (int rc = seg_sums<FIELD_SIDE_LANES>(c, c->fiSide, 2 * n, nC, side, o.side))
        return rc;
    HIPCK(hipGetLastError());
    return DEME_OK;
}
// the asked columns on the host, before they are handed to the caller
struct FieldHost {
    std::vector<uint32_t> clumps, sides;
    std::vector<double> mass, volume, momentum, kinetic, virial;
    uint64_t bytes = 0;  // of the asked columns
    FieldHost(const DemeFieldColumns* a, size_t nC)
        : clumps(a->clumps ? nC : 0), sides(a->sides ? nC : 0), mass(a->mass ? nC : 0), volume(a->volume ? nC : 0),
          momentum(a->momentum ? 3 * nC : 0), kinetic(a->kinetic ? 6 * nC : 0), virial(a->virial ? 9 * nC : 0) {
        bytes = 4 * (uint64_t)(clumps.size() + sides.size()) + 8 * (uint64_t)(mass.size() + volume.size() + momentum.size() + kinetic.size() + virial.size());
    }
    void add(const FieldHost& h) {
        auto sum = [](auto& a, const auto& b) {
            for (size_t i = 0; i < a.size(); i++)
                a[i] += b[i];
        };
        sum(clumps, h.clumps), sum(sides, h.sides), sum(mass, h.mass), sum(volume, h.volume), sum(momentum, h.momentum), sum(kinetic, h.kinetic),
            sum(virial, h.virial);
    }
    void hand_over(const DemeFieldColumns* a) const {
        auto copy = [](auto* dst, const auto& v) {
            if (dst && !v.empty())
                memcpy(dst, v.data(), v.size() * sizeof v[0]);
        };
        copy(a->clumps, clumps), copy(a->sides, sides), copy(a->mass, mass), copy(a->volume, volume), copy(a->momentum, momentum),
            copy(a->kinetic, kinetic), copy(a->virial, virial);
    }
};
// the asked columns of the sums fields_launch left, to h; waits for the stream
int fields_fetch(deme_ctx* c, size_t nC, FieldHost& h) {
    const FieldOutDev o = fields_out(c, nC);
    auto get = [&](auto& v, const void* src) -> hipError_t {
        return v.empty() ? hipSuccess : hipMemcpyAsync(v.data(), src, v.size() * sizeof v[0], hipMemcpyDeviceToHost, c->stream);
    };
    HIPCK(get(h.clumps, o.own.clumps));
    HIPCK(get(h.sides, o.side.sides));
    HIPCK(get(h.mass, o.own.mass));
    HIPCK(get(h.volume, o.own.volume));
    HIPCK(get(h.momentum, o.own.momentum));
    HIPCK(get(h.kinetic, o.own.kinetic));
    HIPCK(get(h.virial, o.side.virial));
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

unsigned deme_fields_block_rows(void) { return SEG_BLOCK_ROWS; }

int deme_inspect_fields(deme_ctx* c, const DemeFieldGrid* grid, float thr, const DemeFieldColumns* out) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = fields_args_refused(msg, "deme_inspect_fields", grid, thr, out))
        return fail(c, rc, "%s", msg);
    if (int rc = fields_ctx_refused(c, out))
        return rc;
    if (int rc = fields_launch(c, grid, thr, fields_ask_owner(out), fields_ask_contact(out)))
        return rc;
    const size_t nC = (size_t)grid->n[0] * grid->n[1] * grid->n[2];
    FieldHost h(out, nC);  // (the caller's arrays are written once the call cannot fail any more)
    if (int rc = fields_fetch(c, nC, h))
        return rc;
    c->qHostBytes += h.bytes;
    h.hand_over(out);
    return DEME_OK;
}

// ---- connected components of the contact network (deme_clusters.h) ---------------------------------------------------------------------
namespace {
static_assert(sizeof(DemeClusterSummary) == sizeof(ClusterStat), "DemeClusterSummary is the device's ClusterStat");
constexpr size_t CLUSTER_ROW_BYTES = 40;  // of clTable: label, size, mass and three moments a row
struct ClusterAsk {
    bool summary, labels, rows, table;  // rows: the row count of the table (asked with the table, or alone)
};
// what deme_inspect_clusters refuses of its arguments alone, in the order it does (the text goes to msg)
int clusters_args_refused(char (&msg)[320], const char* who, const void* summary, const void* labels, size_t labelCap, size_t nOwners,
                          const void* table, const void* nClusters, float thr) {
    msg[0] = 0;
    if (!summary && !labels && !table && !nClusters)
        snprintf(msg, sizeof msg, "%s: null output (summary, labels, table and nClusters)", who);
    else if (labels && labelCap < nOwners)
        snprintf(msg, sizeof msg, "%s: buffer too small: need %zu labels", who, nOwners);
    else
        threshold_refused(msg, who, thr);
    return msg[0] ? DEME_ERR_INVALID : DEME_OK;
}
// what one context refuses of a question whose arguments are in order (the text is left in c->err)
int clusters_ctx_refused(deme_ctx* c) {
    if (int rc = records_refused(c))
        return rc;
    if (c->haveList && c->nContacts >= ((uint64_t)1 << 31))
        return fail(c, DEME_ERR_INVALID, "the list has %llu rows; the rows are indexed with 32 bits", (unsigned long long)c->nContacts);
    return DEME_OK;
}
// the columns of the table in clTable (nO rows at the most: a cluster has a counted owner)
ClusterTableOut clusters_table(deme_ctx* c, size_t nO) {
    char* b = c->clTable.as<char>();
    ClusterTableOut o;
    o.rank = c->clRank.as<uint32_t>();
    o.label = reinterpret_cast<uint32_t*>(b), o.size = o.label + nO;
    o.mass = reinterpret_cast<double*>(b + 8 * nO), o.moment = o.mass + nO;
    return o;
}
// where the summary is left in clStat: behind the link pass's edge partials and the stats pass's partials
ClusterStat* clusters_stat_partials(deme_ctx* c, unsigned gridL) { return reinterpret_cast<ClusterStat*>(c->clStat.as<char>() + (((size_t)gridL * 4 + 7) & ~(size_t)7)); }
unsigned clusters_grid_link(deme_ctx* c) { return grid_for(c->haveList ? (size_t)c->nContacts : 0); }
unsigned clusters_grid_stats(deme_ctx* c) { return grid_for(std::max<size_t>(std::max<size_t>(c->nOwners, clusters_grid_link(c)), 1)); }
// The passes of one context, enqueued on its stream: labels in clLabel (per caller id), the summary in clStat, the row count in
// clCtl, the table in clTable.  ownerGid: a slab of a decomposed run -- its ghost copies link, and an edge is counted by the slab
// that owns the clump with the smaller global id.  Nothing the step reads is written.
int clusters_launch(deme_ctx* c, float thr, const uint32_t* ownerGid, ClusterAsk ask) {
    const size_t nO = c->nOwners, n = c->haveList ? (size_t)c->nContacts : 0;
    const unsigned gridL = clusters_grid_link(c), gridS = clusters_grid_stats(c);
    if (ensure(c, c->clCtl, sizeof(ClusterCtl)) || ensure(c, c->clParent, nO * 4) || ensure(c, c->clLabel, nO * 4) || ensure(c, c->clSize, nO * 4) ||
        ensure(c, c->clStat, (((size_t)gridL * 4 + 7) & ~(size_t)7) + ((size_t)gridS + 1) * sizeof(ClusterStat)))
        return c->lastStatus;
    // (the sorted half of the pairs is reserved only when the table is asked)
    if (ask.rows && (ensure(c, c->clFlag, nO * 4) || ensure(c, c->clRank, nO * 4) || seg_reserve(c, c->clSel, nO, ask.table)))
        return c->lastStatus;
    if (ask.table && ensure(c, c->clTable, nO * CLUSTER_ROW_BYTES))
        return c->lastStatus;
    HIPCK(hipMemsetAsync(c->clCtl.p, 0, sizeof(ClusterCtl), c->stream));
    ClusterCtl* ctl = c->clCtl.as<ClusterCtl>();
    uint32_t *parent = c->clParent.as<uint32_t>(), *label = c->clLabel.as<uint32_t>(), *size = c->clSize.as<uint32_t>();
    const OwnerRec* owners = c->owners.as<OwnerRec>();
    {
        ScopedTimer tm(c, "clusters_label", true);
        if (nO)
            hipLaunchKernelGGL(k_cluster_init, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, c->nOwnerClumps, owners, c->dp.o2e,
                               ownerGid ? 1 : 0, parent, size);
        if (nO && n) {
            ClusterLinkArgs a{};
            a.n = (uint32_t)n, a.nSlots = (uint32_t)nO, a.keys = c->keysSorted[c->keysCur].as<uint64_t>();
            a.t = query_tables(c), a.owners = owners, a.o2e = c->dp.o2e, a.force = c->rec[0].as<float>(), a.thr2 = threshold_sq(thr);
            a.parent = parent, a.ownerGid = ownerGid, a.edgePartial = c->clStat.as<uint32_t>(), a.ctl = ctl;
            hipLaunchKernelGGL(k_cluster_link, dim3(gridL), dim3(256), 0, c->stream, a);
        }
        if (nO)
            hipLaunchKernelGGL(k_cluster_flatten, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, owners, c->dp.o2e, parent, label, size, ctl);
        if (ask.summary) {
            ClusterStat* partial = clusters_stat_partials(c, gridL);
            hipLaunchKernelGGL(k_cluster_stats, dim3(gridS), dim3(256), 0, c->stream, (uint32_t)nO, label, size, nO && n ? gridL : 0u,
                               c->clStat.as<uint32_t>(), partial);
            hipLaunchKernelGGL(k_cluster_stats_final, dim3(1), dim3(256), 0, c->stream, gridS, partial, partial + gridS);
        }
    }
    if (!nO || !ask.rows) {
        HIPCK(hipGetLastError());
        return DEME_OK;
    }
    {
        ScopedTimer tm(c, "clusters_sort", true);
        hipLaunchKernelGGL(k_cluster_select, dim3(grid_for(nO)), dim3(256), 0, c->stream, (uint32_t)nO, owners, c->dp.o2e, label, size,
                           c->clSel.key[0].as<uint32_t>(), c->clSel.val[0].as<uint32_t>(), c->clFlag.as<uint32_t>());
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(DEME_SCAN_T), 0, c->stream, c->clFlag.as<uint32_t>(), c->clRank.as<uint32_t>(), (uint32_t)nO,
                           &ctl->nRows);
        if (ask.table)
            if (int rc = seg_sort(c, c->clSel, nO, nO))
                return rc;
    }
    if (ask.table) {
        ScopedTimer tm(c, "clusters_sums", true);
        if (int rc = seg_sums<CLUSTER_LANES>(c, c->clSel, nO, nO, ClusterTerm{c->dp, c->clSel.val[1].as<uint32_t>(), owners, c->massProps.as<float4>()},
                                             clusters_table(c, nO)))
            return rc;
    }
    HIPCK(hipGetLastError());
    return DEME_OK;
}
// the control words and, if asked, the summary clusters_launch left; waits for the stream.  A bound that fired is an error.
int clusters_fetch_head(deme_ctx* c, bool summary, ClusterCtl* ctl, DemeClusterSummary* sum) {
    HIPCK(hipMemcpyAsync(ctl, c->clCtl.p, sizeof *ctl, hipMemcpyDeviceToHost, c->stream));
    if (summary)
        HIPCK(hipMemcpyAsync(sum, clusters_stat_partials(c, clusters_grid_link(c)) + clusters_grid_stats(c), sizeof *sum, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->clRetries = ctl->retries;
    if (ctl->bound)
        return fail(c, DEME_ERR_INTERNAL, "the cluster labelling ran into its bound of %u steps: the forest of parents is damaged (a defect of "
                    "the library, not of the call)", c->nOwners);
    return DEME_OK;
}
// the table's rows on the host, before they are handed to the caller
struct ClusterRows {
    std::vector<uint32_t> label, size;
    std::vector<double> mass, moment;
    uint64_t bytes = 0;
    ClusterRows(bool l, bool s, bool m, bool mo, size_t rows) : label(l ? rows : 0), size(s ? rows : 0), mass(m ? rows : 0), moment(mo ? 3 * rows : 0) {
        bytes = 4 * (uint64_t)(label.size() + size.size()) + 8 * (uint64_t)(mass.size() + moment.size());
    }
};
// enqueues the copies of the asked columns of the first rows.label.size() ... rows; the caller waits
int clusters_fetch_rows(deme_ctx* c, ClusterRows& h) {
    const ClusterTableOut o = clusters_table(c, c->nOwners);
    auto get = [&](auto& v, const void* src) -> hipError_t {
        return v.empty() ? hipSuccess : hipMemcpyAsync(v.data(), src, v.size() * sizeof v[0], hipMemcpyDeviceToHost, c->stream);
    };
    HIPCK(get(h.label, o.label));
    HIPCK(get(h.size, o.size));
    HIPCK(get(h.mass, o.mass));
    HIPCK(get(h.moment, o.moment));
    return DEME_OK;
}
}  // namespace

int deme_inspect_clusters(deme_ctx* c, float thr, DemeClusterSummary* summary, uint32_t* labels, size_t labelCap, const DemeClusterColumns* table,
                          size_t tableCap, size_t* nClusters) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = clusters_args_refused(msg, "deme_inspect_clusters", summary, labels, labelCap, c->nOwners, table, nClusters, thr))
        return fail(c, rc, "%s", msg);
    if (int rc = clusters_ctx_refused(c))
        return rc;
    const ClusterAsk ask{summary != nullptr, labels != nullptr, table || nClusters, table != nullptr};
    if (int rc = clusters_launch(c, thr, nullptr, ask))
        return rc;
    ClusterCtl ctl{};
    DemeClusterSummary sum{};
    if (int rc = clusters_fetch_head(c, ask.summary, &ctl, &sum))
        return rc;
    c->qHostBytes += sizeof ctl + (ask.summary ? sizeof sum : 0);
    const size_t nO = c->nOwners, rows = ask.rows ? (size_t)ctl.nRows : 0;
    if (nClusters)
        *nClusters = rows;
    if (table && tableCap < rows)
        return fail(c, DEME_ERR_INVALID, "deme_inspect_clusters: the table has %zu rows; room for %zu was given", rows, tableCap);
    std::vector<uint32_t> hl(labels ? nO : 0);  // (the caller's arrays are written once the call cannot fail any more)
    ClusterRows h(table && table->label, table && table->size, table && table->mass, table && table->moment, rows);
    if (!hl.empty())
        HIPCK(hipMemcpyAsync(hl.data(), c->clLabel.p, nO * 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = clusters_fetch_rows(c, h))
        return rc;
    HIPCK(hipStreamSynchronize(c->stream));
    c->qHostBytes += 4ull * hl.size() + h.bytes;
    if (summary)
        *summary = sum;
    if (!hl.empty())
        memcpy(labels, hl.data(), nO * 4);
    auto copy = [](auto* dst, const auto& v) {
        if (dst && !v.empty())
            memcpy(dst, v.data(), v.size() * sizeof v[0]);
    };
    if (table)
        copy(table->label, h.label), copy(table->size, h.size), copy(table->mass, h.mass), copy(table->moment, h.moment);
    return DEME_OK;
}

int deme_clusters_link_retries(const deme_ctx* c, uint64_t* retries) {
    if (!c || !retries)
        return DEME_ERR_INVALID;
    *retries = c->clRetries;
    return DEME_OK;
}

// ---- pose, velocity and family of a few owners (deme_query.h: k_query_owner_state) ------------------------------------------------
namespace {
// the columns of DemeOwnerState a gathered record fills: row `at` of every non-null column from record r
inline void owner_state_row(const DemeOwnerState* out, size_t at, const OwnerRec& r) {
#define DEME_COL(abi, T, Rec, f) if (out->abi) out->abi[at] = r.f;
    DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL_NONE)
#undef DEME_COL
    if (out->familyID) out->familyID[at] = (uint8_t)r.family;
}
}  // namespace

int deme_query_owner_state(deme_ctx* c, const uint32_t* ownerIds, size_t n, DemeOwnerState* out) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    if (int rc = owner_ids_refused(msg, "deme_query_owner_state", out, "state", ownerIds, n, c->nOwners, out,
                                   "need the reduction a full download launches (deme_download_owner_state)", true))
        return fail(c, rc, "%s", msg);
    if (!n)
        return DEME_OK;
    std::vector<uint32_t> slots(n);
    for (size_t i = 0; i < n; i++)
        slots[i] = c->permuted ? c->hE2O[ownerIds[i]] : ownerIds[i];
    if (ensure(c, c->stage, n * 4) || ensure(c, c->qState, n * sizeof(OwnerRec)))
        return c->lastStatus;
    HIPCK(hipMemcpyAsync(c->stage.p, slots.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_query_owner_state, dim3(grid_for(n)), dim3(256), 0, c->stream, (uint32_t)n, c->owners.as<OwnerRec>(),
                       c->stage.as<uint32_t>(), (const uint32_t*)nullptr, SlabBooksDev{}, 0u, 0u, (const uint8_t*)nullptr,
                       c->qState.as<OwnerRec>(), (uint32_t)n, (uint32_t*)nullptr);
    std::vector<OwnerRec> h(n);
    HIPCK(hipMemcpyAsync(h.data(), c->qState.p, n * sizeof(OwnerRec), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    c->qHostBytes += (uint64_t)n * sizeof(OwnerRec);
    for (size_t i = 0; i < n; i++)
        owner_state_row(out, i, h[i]);
    return DEME_OK;
}

// ---- writing them (deme_query.h: k_scatter_owner_state) ---------------------------------------------------------------------------
namespace {
// the columns a call gave as the kernel's mask, and row `at` of them as the record the kernel reads its values from
inline uint32_t owner_state_mask(const DemeOwnerState* in) {
#define DEME_COL(abi, T, Rec, f) | (in->abi ? DEME_SCATTER_BIT(abi) : 0u)
    return 0u DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL);
#undef DEME_COL
}
inline OwnerRec owner_state_patch(const DemeOwnerState* in, size_t at) {
    OwnerRec r{};
#define DEME_COL(abi, T, Rec, f) if (in->abi) r.f = in->abi[at];
    DEME_OWNER_COLS(DEME_COL, DEME_COL_NONE, DEME_COL)  // (the family's byte alone: the kernel keeps the record's flag bits)
#undef DEME_COL
    return r;
}
// keys (4 bytes each) and records (64 bytes each) to the device, the kernel, and the wait that lets the host arrays go
// (the flags of a write of `in`'s columns are set once the scratch is there: a call that fails before it has changed nothing)
int launch_owner_scatter(deme_ctx* c, const DemeOwnerState* in, const std::vector<uint32_t>& keys, const std::vector<OwnerRec>& patch,
                         uint32_t mask, bool byGid, const uint32_t* ownerGid) {
    const size_t n = keys.size();
    if (ensure(c, c->stage, n * 4) || ensure(c, c->qState, n * sizeof(OwnerRec)))
        return c->lastStatus;
    owner_state_written(c, in);
    HIPCK(hipMemcpyAsync(c->stage.p, keys.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCK(hipMemcpyAsync(c->qState.p, patch.data(), n * sizeof(OwnerRec), hipMemcpyHostToDevice, c->stream));
    const uint32_t threads = byGid ? c->nOwners : (uint32_t)n;
    if (threads)
        hipLaunchKernelGGL(k_scatter_owner_state, dim3(grid_for(threads)), dim3(256), 0, c->stream, threads, c->owners.as<OwnerRec>(), c->nOwners,
                           c->stage.as<uint32_t>(), (uint32_t)n, c->qState.as<OwnerRec>(), mask, byGid ? c->dp.o2e : (const uint32_t*)nullptr,
                           byGid ? ownerGid : (const uint32_t*)nullptr);
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

int deme_scatter_owner_state(deme_ctx* c, const uint32_t* ownerIds, size_t n, const DemeOwnerState* in) {
    if (int rc = check_ready(c))
        return rc;
    char msg[320];
    std::vector<std::pair<uint32_t, uint32_t>> sorted;
    if (int rc = owner_ids_refused(msg, "deme_scatter_owner_state", in, "state", ownerIds, n, c->nOwners, in,
                                   "columns are not written by owner id (deme_upload_owner_state hands the accumulators to the caller)", true, &sorted))
        return fail(c, rc, "%s", msg);
    const uint32_t mask = owner_state_mask(in);
    if (!n || !mask)
        return DEME_OK;
    std::vector<uint32_t> slots(n);
    std::vector<OwnerRec> patch(n);
    for (size_t i = 0; i < n; i++) {
        slots[i] = c->permuted ? c->hE2O[ownerIds[i]] : ownerIds[i];
        patch[i] = owner_state_patch(in, i);
    }
    if (int rc = launch_owner_scatter(c, in, slots, patch, mask, false, nullptr))
        return rc;
    c->qHostBytes += (uint64_t)n * (4 + sizeof(OwnerRec));
    return DEME_OK;
}

// ---- the radix sort alone, on host arrays (tests/test_radix_sort.py) -----------------------------
namespace {
struct SortScratch {  // device copies of one call's arrays, freed however the call ends
    std::vector<void*> held;
    ~SortScratch() {
        for (void* p : held)
            (void)hipFree(p);
    }
    template <typename T>
    T* room(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess)
            return nullptr;
        held.push_back(p);
        return reinterpret_cast<T*>(p);
    }
};
template <class RocCfg, bool HAS_V, typename K>
int sort_host_arrays(int device, const K* keys, const uint32_t* vals, size_t n, unsigned beginBit, unsigned endBit, size_t ownFrom, K* keysOut,
                     uint32_t* valsOut) {
    if (endBit < beginBit || endBit > 8 * sizeof(K) || (n && (!keys || !keysOut || (HAS_V && (!vals || !valsOut)))))
        return DEME_ERR_INVALID;
    if (!ownFrom && (DEME_SORT_ROCPRIM || n > deme_sort::MAX_N))  // the own sort was asked for and this build or size has none
        return DEME_ERR_INVALID;
    if (!n)
        return DEME_OK;
    if (hipSetDevice(device) != hipSuccess)
        return DEME_ERR_HIP;
    SortScratch s;
    K *dIn = s.room<K>(n), *dOut = s.room<K>(n);
    uint32_t *vIn = HAS_V ? s.room<uint32_t>(n) : nullptr, *vOut = HAS_V ? s.room<uint32_t>(n) : nullptr;
    if (!dIn || !dOut || (HAS_V && (!vIn || !vOut)))
        return DEME_ERR_HIP;
    size_t bytes = 0;
    if (deme_radix_sort<RocCfg, HAS_V>(nullptr, bytes, dIn, dOut, vIn, vOut, n, n, beginBit, endBit, ownFrom, nullptr) != hipSuccess)
        return DEME_ERR_HIP;
    void* tmp = s.room<char>(bytes);
    if (!tmp)
        return DEME_ERR_HIP;
    bool ok = hipMemcpy(dIn, keys, n * sizeof(K), hipMemcpyHostToDevice) == hipSuccess;
    if (HAS_V)
        ok = ok && hipMemcpy(vIn, vals, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && deme_radix_sort<RocCfg, HAS_V>(tmp, bytes, dIn, dOut, vIn, vOut, n, n, beginBit, endBit, ownFrom, nullptr) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    ok = ok && hipMemcpy(keysOut, dOut, n * sizeof(K), hipMemcpyDeviceToHost) == hipSuccess;
    if (HAS_V)
        ok = ok && hipMemcpy(valsOut, vOut, n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    return ok ? DEME_OK : DEME_ERR_HIP;
}
}  // namespace

unsigned deme_sort_tile_keys(void) { return deme_sort::TILE; }

int deme_sort_pairs_u32(int device, const uint32_t* keys, const uint32_t* vals, size_t n, unsigned beginBit, unsigned endBit, int forceOwn,
                        uint32_t* keysOut, uint32_t* valsOut) {
    const unsigned bits = endBit >= beginBit ? endBit - beginBit : 0;
    if (bits <= 20)  // the short keys of the crossing records
        return sort_host_arrays<DemeRadixCfg<10>, true>(device, keys, vals, n, beginBit, endBit, forceOwn ? 0 : DEME_SORT_OWN_FROM_RECORDS, keysOut,
                                                        valsOut);
    if (bits <= 22)  // (the incidence sort's two configurations)
        return sort_host_arrays<DemeRadixCfg<11, 16>, true>(device, keys, vals, n, beginBit, endBit, forceOwn ? 0 : DEME_SORT_OWN_FROM_INCIDENCES,
                                                            keysOut, valsOut);
    return sort_host_arrays<DemeRadixCfg<8>, true>(device, keys, vals, n, beginBit, endBit, forceOwn ? 0 : DEME_SORT_OWN_FROM_INCIDENCES, keysOut,
                                                   valsOut);
}

int deme_sort_keys_u64(int device, const uint64_t* keys, size_t n, unsigned beginBit, unsigned endBit, int forceOwn, uint64_t* keysOut) {
    return sort_host_arrays<DemeRadixCfg<8>, false>(device, keys, nullptr, n, beginBit, endBit, forceOwn ? 0 : DEME_SORT_OWN_FROM_KEYS64, keysOut,
                                                    nullptr);
}

// ---- the segmented sum alone, on host arrays (tests/test_seg_sum.py) ------------------------------
namespace {
struct CtxHeld {  // a context of one call's own (its stream, segPartial), destroyed however the call ends
    deme_ctx* c = nullptr;
    ~CtxHeld() {
        if (c)
            deme_ctx_destroy(c);
    }
};
template <int L>
int seg_sum_host_arrays(int device, const uint32_t* keys, const double* terms, size_t n, uint32_t nKeys, double* sums, uint32_t* counts) {
    CtxHeld h;
    if (int rc = deme_ctx_create(device, &h.c))
        return rc;
    deme_ctx* c = h.c;
    SortScratch s;
    uint32_t *dKeys = s.room<uint32_t>(n), *dCounts = s.room<uint32_t>(nKeys);
    double *dTerms = s.room<double>(n * L), *dSums = s.room<double>((size_t)nKeys * L);
    if (!dKeys || !dCounts || !dTerms || !dSums)
        return DEME_ERR_HIP;
    if (n) {
        HIPCK(hipMemcpyAsync(dKeys, keys, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(dTerms, terms, n * L * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipMemsetAsync(dSums, 0, (size_t)nKeys * L * 8, c->stream));
    HIPCK(hipMemsetAsync(dCounts, 0, (size_t)nKeys * 4, c->stream));
    if (int rc = seg_sums<L>(c, dKeys, n, nKeys, SegArrayTerm<L>{dTerms}, SegArrayOut<L>{dSums, dCounts}))
        return rc;
    HIPCK(hipGetLastError());
    if (nKeys) {
        HIPCK(hipMemcpyAsync(sums, dSums, (size_t)nKeys * L * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCK(hipMemcpyAsync(counts, dCounts, (size_t)nKeys * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCK(hipStreamSynchronize(c->stream));
    return DEME_OK;
}
}  // namespace

int deme_seg_sum_f64(int device, const uint32_t* keys, const double* terms, size_t n, unsigned lanes, uint32_t nKeys, double* sums,
                     uint32_t* counts) {
    if (n >= ((size_t)1 << 31) || (n && (!keys || !terms)) || (nKeys && (!sums || !counts)))
        return DEME_ERR_INVALID;
    for (size_t i = 1; i < n; i++)  // (this input comes from outside: the kernels rely on the ascent)
        if (keys[i] < keys[i - 1])
            return DEME_ERR_INVALID;
    switch (lanes) {  // the instantiated widths: the inspectors'
        case TRI_LANES: return seg_sum_host_arrays<TRI_LANES>(device, keys, terms, n, nKeys, sums, counts);
        case CLUSTER_LANES: return seg_sum_host_arrays<CLUSTER_LANES>(device, keys, terms, n, nKeys, sums, counts);
        case FIELD_SIDE_LANES: return seg_sum_host_arrays<FIELD_SIDE_LANES>(device, keys, terms, n, nKeys, sums, counts);
        case FIELD_OWNER_LANES: return seg_sum_host_arrays<FIELD_OWNER_LANES>(device, keys, terms, n, nKeys, sums, counts);
    }
    return DEME_ERR_INVALID;
}

#include "deme_decomp.inc"
