/*
 * deme_hip.h -- C-ABI of the MI355X-native DEM hot path (libdeme_hip.so).
 *
 * The reference (projectchrono/DEM-Engine) has no C ABI: its host classes call
 * C++ functions and runtime-compiled CUDA kernels directly.  Each entry point
 * below names the reference interface it replaces (paths relative to the
 * reference tree, src/...).  Plain pointers and sizes only; no C++ or torch
 * types cross this boundary; no exception crosses it (every call returns an
 * int status, 0 = OK, and deme_last_error() gives the message).
 *
 * One context per GPU.  Calls on one context must be serialised by the caller.
 * All work is enqueued on the context's HIP stream (deme_ctx_set_stream lets a
 * caller such as PyTorch hand in its own stream).
 */
#ifndef DEME_HIP_H
#define DEME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants (reference: DEM/Defines.h:74-82, 99-112, 146) ------------- */
#define DEME_NOT_A_CONTACT 0
#define DEME_SPHERE_SPHERE_CONTACT 1
#define DEME_SPHERE_MESH_CONTACT 2
#define DEME_SPHERE_PLANE_CONTACT 11
#define DEME_SPHERE_CYL_CONTACT 13

#define DEME_ANAL_OBJ_TYPE_PLANE 0
#define DEME_ANAL_OBJ_TYPE_PLATE 1
#define DEME_ANAL_OBJ_TYPE_CYL_INF 2

#define DEME_NULL_MAPPING_PARTNER 0xFFFFFFFFu
#define DEME_NULL_BINID 0xFFFFFFFFu
#define DEME_NUM_FAMILIES 256
#define DEME_FAMILY_MASK_ENTRIES 32896 /* 256*257/2, DEM/kT.cpp:609 */
#define DEME_MAX_WILDCARD_NUM 16

#define DEME_INTEGRATOR_FORWARD_EULER 0
#define DEME_INTEGRATOR_CENTERED_DIFFERENCE 1
#define DEME_INTEGRATOR_EXTENDED_TAYLOR 2

#define DEME_FORCE_HERTZIAN 0              /* FullHertzianForceModel.cu: 4 contact wildcards */
#define DEME_FORCE_HERTZIAN_FRICTIONLESS 1 /* FrictionlessHertzianForceModel.cu: 0 wildcards */
#define DEME_FORCE_CUSTOM 2                /* user fragment, see deme_compile_force_model */

/* familyFlags bits: data-driven form of the prescription `switch` the
 * reference JIT-compiles into integrateOwners (DEMIntegrationKernels.cu:26-33,
 * APIPublic.cpp:980-1011 SetFamilyFixed). */
#define DEME_FAMILY_FIXED 1
/* (retired: ghost copies are marked per owner, DemeScene.ownerGhost, and keep their own family) */
#define DEME_FAMILY_GHOST 2
#define DEME_FAMILY_PRESCRIBED 4 /* the family has a compiled motion prescription (deme_compile_prescriptions) */

/* status codes */
#define DEME_OK 0
#define DEME_ERR_INVALID 1
#define DEME_ERR_HIP 2
#define DEME_ERR_OVERFLOW 3 /* an arena (incidences / contacts) was too small even after growth */
#define DEME_ERR_BIN_TOO_FULL 4 /* reference: errOutBinSphNum abort, DEMContactKernels_SphereSphere.cu:121 */
#define DEME_ERR_VELOCITY 5     /* reference: errOutVel, kT.cpp:136-149 */
#define DEME_ERR_COMPILE 6
#define DEME_ERR_PEER 7 /* a collective call gave up because ANOTHER rank of the halo group reported an error (its own message says which) */
#define DEME_ERR_HALO 8 /* deme_multi_change_owner_sizes: the grown clumps would no longer fit the halo the slabs were cut with */
#define DEME_ERR_INTERNAL 9 /* a bounded device loop ran into its bound (deme_inspect_clusters): a defect of the library, not of the call */

/* ---- parameter block: replaces deme::DEMSimParams (DEM/Defines.h:194-265) - */
typedef struct DemeParams {
    uint32_t nvXp2, nvYp2, nvZp2; /* voxel-count bit split, APIPrivate.cpp:373-487 */
    uint32_t nbX, nbY, nbZ;       /* bins per axis, HostSideHelpers.hpp:195-207 */
    double l;                     /* sub-voxel length unit */
    double voxelSize;             /* 2^16 * l */
    double binSize;
    float LBFX, LBFY, LBFZ; /* left-bottom-front corner of the world */
    float Gx, Gy, Gz;
    float h;              /* time step */
    float beta;           /* constant radius inflation (SetExpandFactor) */
    float approxMaxVel;   /* cap used by the margin formula, DEMMiscKernels.cu:50 */
    float expSafetyMulti; /* margin = (min(v,cap)*multi+adder)*h*drift + familyExtra */
    float expSafetyAdder;
    uint32_t integrator;        /* DEME_INTEGRATOR_* */
    uint32_t forceModel;        /* DEME_FORCE_* */
    uint32_t nContactWildcards; /* 4 for Hertzian, 0 frictionless, user value for custom */
    uint32_t cdUpdateFreq;      /* contact detection every K steps; 0 = every step with zero margin
                                   (the reference's SetCDUpdateFreq(0) parity mode) */
    uint32_t errOutBinSphNum;   /* default 32768 */
    float errOutVel;            /* default 1e15 (DEME_HUGE_FLOAT) */
    double timeElapsed;
} DemeParams;

/* ---- model description: replaces the DEMDataKT/DEMDataDT struct-of-pointers
 * (DEM/Defines.h:269-428) plus the JIT constant tables (_clumpTemplateDefs_,
 * _massDefs_, _moiDefs_, _analyticalEntityDefs_, _materialDefs_).
 * All pointers are HOST pointers, copied at upload time.  Owner order: clumps,
 * then analytical objects, then meshes (kT.cpp:804-829).  Sphere order is
 * clump-major. */
typedef struct DemeScene {
    uint32_t nOwners, nOwnerClumps, nSpheres, nAnal, nTri, nMat, nComp, nMassProps;
    /* per owner */
    const uint64_t* voxelID;
    const uint16_t *locX, *locY, *locZ;
    const float *oriQw, *oriQx, *oriQy, *oriQz;
    const float *vX, *vY, *vZ;
    const float *omgBarX, *omgBarY, *omgBarZ;
    const uint8_t* familyID;
    const uint16_t* inertiaPropOffsets;
    /* per sphere */
    const uint32_t* ownerClumpBody;
    const uint16_t* clumpComponentOffset;
    const uint16_t* sphereMaterialOffset;
    /* clump component tables (nComp) and mass-property tables (nMassProps) */
    const float *Radii, *CDRelPosX, *CDRelPosY, *CDRelPosZ;
    const float *MassProperties, *moiX, *moiY, *moiZ;
    /* analytical components (nAnal), AnalyticalCompDefJitify.cu:2-15 */
    const uint8_t* objType;
    const uint32_t* objOwner;
    const float* objNormal; /* +1 inward, -1 outward */
    const uint16_t* objMaterial;
    const float *objRelPosX, *objRelPosY, *objRelPosZ;
    const float *objRotX, *objRotY, *objRotZ;
    const float *objSize1, *objSize2, *objSize3;
    const float* objMass;
    /* materials: E[nMat], nu[nMat]; CoR/mu/Crr are nMat*nMat row-major (APIPrivate.cpp:1877-2026) */
    const float *E, *nu, *CoR, *mu, *Crr;
    /* families */
    const uint8_t* familyMasks;         /* DEME_FAMILY_MASK_ENTRIES, DEMHelperKernels.cuh:58-62 */
    const float* familyExtraMarginSize; /* 256 */
    const uint8_t* familyFlags;         /* 256, DEME_FAMILY_* bits */
    /* triangles (nTri): mesh-major, owner-local node coordinates, APIPrivate.cpp:756-810 */
    const uint32_t* ownerMesh;
    const float *triNode1, *triNode2, *triNode3; /* nTri*3 floats each, xyz interleaved */
    const uint16_t* triMaterialOffset;
    /* per owner, may be NULL: 1 = a ghost copy of a clump that another rank owns and integrates (slab decomposition, SURVEY
     * 8e).  A ghost keeps its TRUE family -- contact masks and family margins apply across a cut as inside a slab -- and is
     * refreshed from its owner rank every step (family included); ghost-ghost pairs are left to the ranks that own them.
     * 2 = a replicated owner that moves under contact forces (a free mesh or analytical body kept on every slab): each slab
     * sums the contributions of the spheres it owns (a ghost sphere's contact with it is left to the sphere's own rank), and
     * deme_halo_group_step adds the per-slab sums up (one ncclAllReduce of 8 floats per such owner) before every replica is
     * integrated with the total.  A context holding such owners can only be stepped through a halo group. */
    const uint8_t* ownerGhost;
} DemeScene;

/* mutable owner state for download/upload round trips */
typedef struct DemeOwnerState {
    uint64_t* voxelID;
    uint16_t *locX, *locY, *locZ;
    float *oriQw, *oriQx, *oriQy, *oriQz;
    float *vX, *vY, *vZ;
    float *omgBarX, *omgBarY, *omgBarZ;
    float *aX, *aY, *aZ;
    float *alphaX, *alphaY, *alphaZ;
    uint8_t* familyID;
} DemeOwnerState;

typedef struct DemeCounts {
    uint64_t nContacts;        /* current contact list length */
    uint64_t nPrevContacts;    /* previous list length (history source) */
    uint64_t nBinSphereTouches;/* (bin, sphere) incidences in the last detection */
    uint64_t nActiveBins;
    uint64_t nSteps;           /* steps taken since creation */
    uint64_t nDetections;
    uint32_t maxSpheresInBin;
    uint32_t lastStatus;
} DemeCounts;

typedef struct deme_ctx deme_ctx;

/* lifecycle.  Replaces DEMKinematicThread/DEMDynamicThread construction
 * (DEM/APIPublic.cpp:22-72) -- one object, one stream, no worker threads. */
int deme_ctx_create(int device, deme_ctx** out);
void deme_ctx_destroy(deme_ctx* ctx);
const char* deme_last_error(const deme_ctx* ctx);
const char* deme_version(void);
int deme_ctx_set_stream(deme_ctx* ctx, void* hip_stream); /* NULL = context-owned stream */
int deme_sync(deme_ctx* ctx);

/* Arithmetic mode of the per-step kernels.  Contact DETECTION (bin assignments, contact lists, history map) is the same
 * decision code in both modes -- bit-exact against the reference's fp64 predicates.
 *  DEME_ARITH_FAST  (default)  the contact-force kernel works from a per-owner derived view (world position in fp64, world
 *      angular velocity, mass: rewritten by the integrator every step), evaluates contacts in the world frame with 1-ulp
 *      hardware reciprocals / square roots and FMA contraction, and accumulates world-frame forces and torques that the
 *      integrator converts once per owner.  Same formulas as kernel/DEMCalcForceKernels.cu + FullHertzianForceModel.cu,
 *      re-associated: results agree with DEME_ARITH_EXACT to fp32 rounding (tolerance stated in tests/test_fast_mode.py).
 *  DEME_ARITH_EXACT  the reference's operation order and correctly rounded division / square root throughout: owner states
 *      bit-identical to the CPU oracle (the parity suite runs in this mode).
 * The process-wide default can be set with the environment variable DEME_ARITH=exact|fast. */
#define DEME_ARITH_FAST 1
#define DEME_ARITH_EXACT 0
int deme_set_arith_mode(deme_ctx* ctx, int mode);
int deme_get_arith_mode(const deme_ctx* ctx);
/* Which kernel evaluates the contact forces of the current list (what a profile of the stepping loop shows as its dominant
 * kernel): "k_tile_forces<M, MESH>" -- the owner-tile pass of the fast mode, csrc/deme_tile.h; MESH = true when the list holds
 * sphere-triangle contacts, which the mesh variant of the general kernel evaluates first -- , "k_forces_fast<M>" (fast mode, a
 * scene the tile pass does not take: replicated free owners, more than 16 materials, tables beyond 4 KB), "k_calc_forces<M, 0>"
 * (exact mode, contact recording) or "deme_custom_forces_ss" (a run-time compiled model); M = 0 Hertzian with history, 1
 * frictionless.  Also the largest tile's foreign-owner count and local list length of the current list.
 * deme_tile_stats: {tiles, tiles that do not fit the LDS area and are evaluated by k_tile_forces_big -- one workgroup each, the
 * rest of the list stays tiled --, largest halo, largest local list} of the current list (zeros when it is not tiled). */
int deme_tile_stats(const deme_ctx* ctx, uint32_t out[4]);
/* (heavy owners, heavy owners that are not fixed) of the current list: the owners whose sums k_reduce_heavy takes -- more than 256
 * A-side plus B-side entries, or replicated across slabs.  The list's general form (k_owner_ranges) and its tile form
 * (k_owner_ranges_tile) count the entries from different structures and must flag the same owners. */
int deme_heavy_owners(deme_ctx* ctx, uint32_t out[2]);
/* A run-time compiled force model is compiled into the tile pass as well ("deme_custom_tile<MESH>": csrc/deme_jit.h splices the
 * user's statements where the Hertzian block of k_tile_forces is, the reference's vocabulary filled from the staged records,
 * DEMCalcForceKernels.cu:233-251).  A list takes it when its tiles hold at least minContactsPerTile contacts on average (default
 * 320: below that -- single spheres with one or two contacts each -- the general kernel is faster, measured on configs[4]);
 * 0 = always. */
int deme_set_tile_policy(deme_ctx* ctx, uint32_t minContactsPerTileCustom);
int deme_force_kernel_name(const deme_ctx* ctx, char* name, size_t cap, uint32_t* tileMaxHalo, uint32_t* tileMaxList);
/* The one-kernel time step (csrc/deme_tile_step.h, "k_tile_step<M>"): every tile is CLOSED -- it also evaluates the contacts that
 * hold its owners as B from other tiles (a contact that straddles two tiles is evaluated by both, bit-identically) -- so that the
 * tile owns the complete sums of its owners and integrates them in the same launch (calculateForces + integrateOwners of
 * dT.cpp:2424-2447 in one kernel; owners and contact history are double-buffered).  OFF by default: on the packed bed of BASELINE
 * configs[1] the closed tiles stage ~220 foreign owners instead of ~95 and evaluate 1.2x the contacts, and the one launch
 * (143 us) is slower than force pass + integrator (92 + 43 us) -- DESIGN.md 3.7.  Built-in models, FAST arithmetic, no mesh,
 * no ghosts, no prescription / family-rule kernels, no recording; anything else keeps the two-kernel form silently.
 * Where it pays (round 5, profiles/r05/fused_small_beds.txt): beds whose step is two short launches -- 10^4 clumps 0.0258 -> 0.0192
 * ms/step (-26 %), 5x10^4 0.0373 -> 0.0306 (-18 %); at 2x10^5 the closed tiles no longer fit and the two-kernel form runs anyway.
 * on = 2: by size -- the one-kernel step for scenes of at most 10^5 owners (what the C++ shell asks for), the two kernels beyond.
 * Environment DEME_FUSED=2 / 1 / 0 overrides the switch for every context of the process. */
int deme_set_fused_step(deme_ctx* ctx, int on);

/* The engine's own numbering (csrc/deme_order.inc).  Owner and sphere ids at this boundary are ALWAYS the caller's -- load order,
 * as in the reference (DEM/dT.cpp:700-800).  Inside, a scene uploaded in the fast arithmetic mode (no ghosts, built-in force
 * model) whose clumps are not already numbered compactly is kept in box-shaped tiles of 128 clumps (recursive bisection), so that
 * the owner tiles of the force pass are clusters of the bed; every entry point translates.  *reordered = 1 if the current scene is
 * kept that way; spread[0] / [1]: mean surface of the bounding box of 128 consecutive clumps (in squares of one bin edge), in the
 * caller's order / in the engine's (0 when the question was not asked).  deme_set_reorder(ctx, 0) before deme_upload_scene keeps the caller's order (env DEME_REORDER=0
 * does it for the process). */
int deme_get_order(const deme_ctx* ctx, int* reordered, double spread[2]);
int deme_set_reorder(deme_ctx* ctx, int enable);
/* A running simulation drifts away from the order it was given (a mixer, a flow).  The engine watches the tiles of every detection
 * (mean foreign owners per tile, tiles that no longer fit) and renews its order at the start of a detection when they have
 * degraded by half since the last ordering, at most every 20 detections; deme_renew_order does it now.  The caller's ids never
 * change.  Host-driven (positions to the host, the order as at upload, records, the current contact list and its history
 * re-keyed): about a second at 1e6 clumps. */
int deme_renew_order(deme_ctx* ctx);
int deme_order_renewals(const deme_ctx* ctx, uint64_t* n); /* how many times the order was renewed (by the engine or by the call above) */
/* The order itself, without a context or a GPU (host code; tests): order[k] = the caller's clump kept in slot k. */
int deme_order_probe(const DemeParams* p, size_t nClumps, const uint64_t* voxelID, const uint16_t* locX, const uint16_t* locY,
                     const uint16_t* locZ, uint32_t* order, double spread[2]);

/* setSimParams / UpdateSimParams (APIPrivate.cpp:1121, dT.cpp:2463-2466) */
int deme_set_params(deme_ctx* ctx, const DemeParams* p);
/* allocateGPUArrays + initGPUArrays + packDataPointers (APIPrivate.cpp:1169-1290) */
int deme_upload_scene(deme_ctx* ctx, const DemeScene* s);
/* DEMTracker setters / SetTriNodeRelPos analogue: overwrite owner state (n = nOwners) */
int deme_upload_owner_state(deme_ctx* ctx, const DemeOwnerState* st);
int deme_download_owner_state(deme_ctx* ctx, DemeOwnerState* st);
/* SetTriNodeRelPos / DEMTracker::UpdateMesh (APIPublic.cpp:709-730): rewrite nTri*3 floats per node array */
int deme_update_tri_nodes(deme_ctx* ctx, const float* n1, const float* n2, const float* n3);

/* kT unpackMyBuffer margin step (kT.cpp:100-191, DEMMiscKernels.cu:37-61):
 * per-owner margin from |v|; drift = number of steps the list must stay valid.
 * drift 0 => margin = familyExtraMargin only. */
int deme_compute_margins(deme_ctx* ctx, uint32_t drift);
/* direct margin override, n = nOwners (tests) */
int deme_set_margins(deme_ctx* ctx, const float* marginSize);

/* contactDetection() (algorithms/DEMCubContactDetection.cu:38-1123): binning,
 * bin-sorted sweep, sphere-analytical and sphere-triangle detection, history map. */
int deme_detect_contacts(deme_ctx* ctx);
/* dT unpack + migrateEnduringContacts (dT.cpp:1955-1987, 2040-2144): permute
 * contact wildcards through the history map of the last detection. */
int deme_migrate_history(deme_ctx* ctx);
/* calculateForces() (dT.cpp:2146-2214): clear a/alpha, per-contact force, accumulate. */
int deme_calc_forces(deme_ctx* ctx);
/* integrateOwnerMotions() (dT.cpp:2216-2224) */
int deme_integrate(deme_ctx* ctx);
/* DoDynamics inner loop (dT.cpp:2401-2467): nsteps of {detect every K, forces, integrate}. */
int deme_step(deme_ctx* ctx, uint32_t nsteps);
/* The reference runs its contact detection (kT) beside the dynamics (dT) with bounded staleness (kT.cpp:100-216, dT.cpp:1955-2038,
 * 2276-2299).  Here, opt-in: leadSteps = D > 0 makes deme_step start a detection D steps before the list is due -- from a copy of
 * the owner records, on a stream of its own, with margins for the K + D steps between the copy and the end of the new list's
 * service -- while the main stream works through those D steps with the current list; the new list is swapped in when they are
 * enqueued.  No contact is missed; the list holds a few more near-pairs (zero contributions) than a lock-step detection's, so an
 * exact-mode trajectory is the lock-step one.  Needs K > D and a deme_step call of at least D steps at the right moment; scenes
 * with a mesh, ghosts, persistent contacts or the adaptive controllers keep the lock-step detection.  0 switches it off. */
int deme_set_async_detection(deme_ctx* ctx, uint32_t leadSteps);

int deme_get_counts(deme_ctx* ctx, DemeCounts* out);

/* outputs for parity checks (capacity in elements; returns DEME_ERR_INVALID if too small) */
/* (bin, sphere) incidence list in bin-sorted order: binIDsEachSphereTouches_sorted /
 * sphereIDsEachBinTouches_sorted (DEMCubContactDetection.cu:169-186) */
int deme_download_bin_incidence(deme_ctx* ctx, uint32_t* binIDs, uint32_t* sphereIDs, size_t cap);
/* contact list: idGeometryA/B, contactType, contactMapping (Defines.h:306-322) */
int deme_download_contacts(deme_ctx* ctx, uint32_t* idA, uint32_t* idB, uint8_t* type, uint32_t* mapping, size_t cap);
/* contact wildcards, array w (0..nContactWildcards-1), length nContacts */
int deme_download_contact_wildcard(deme_ctx* ctx, uint32_t w, float* out, size_t cap);
int deme_upload_contact_wildcard(deme_ctx* ctx, uint32_t w, const float* in, size_t n);
/* Restart: load a saved contact list with its wildcards (DEMClumpBatch::SetExistingContacts /
 * SetExistingContactWildcards, Structs.h:857-880; loaded by dT at initialisation).  The
 * pairs are geometry ids (sphere A; sphere / triangle / analytical component B), `type` the reference's
 * contact_t (1 SS, 2 SM, other: analytical); `wildcards` is float[n][nContactWildcards].  The list only feeds
 * the history map of the next detection, which therefore always runs before the next force evaluation. */
int deme_seed_contacts(deme_ctx* ctx, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, const float* wildcards,
                       size_t n);
/* per-contact records (ContactInfoWriteBack.cu): force, torque-only force, local contact
 * points; each nContacts*3 floats; any pointer may be NULL. Recording must have been enabled. */
int deme_set_record_contacts(deme_ctx* ctx, int enable);
int deme_download_contact_records(deme_ctx* ctx, float* force, float* torqueOnly, float* cpA, float* cpB, size_t cap);
/* The contacts of a few owners, selected on the device (reference: getContactForcesConcerningOwners,
 * algorithms/DEMDynamicMisc.cu:14-100, DEM/dT.cpp:2740-2852; DEMSolver::GetOwnerContactClumps, DEM/APIPublic.cpp:323-395): every
 * row of the current list whose sphere A or whose geometry B belongs to one of ownerIds (the caller's numbering; a repeated id
 * counts once).  Rows come back in the order deme_download_contacts lists them -- the result is a sub-sequence of that list,
 * whether or not the engine keeps an order of its own -- with idA, idB, type and, when withRecords != 0, the four per-contact
 * records bitwise what deme_download_contacts / deme_download_contact_records give for the same rows; ownerA / ownerB: the owners
 * of the two geometries; side: 0 when A's owner is one of ownerIds, 1 when only B's is.  Any output pointer may be NULL.  *nOut
 * receives the hit count; with cap < *nOut no row is written and the call returns DEME_ERR_INVALID, so a caller asks with cap 0,
 * sizes its arrays and asks again.  Only the count and the hit rows come to the host (24 bytes a row, 72 with records):
 * deme_query_host_bytes reports what these calls have copied since the context was created (4 bytes per count read-back --
 * two when the scratch had to grow -- and the rows).  Refused, with nothing written (nOut included): an owner id out of
 * range; withRecords while recording is off or the list is a seed (the messages of deme_download_contact_records). */
int deme_query_owner_contacts(deme_ctx* ctx, const uint32_t* ownerIds, size_t nOwners, int withRecords, uint32_t* idA, uint32_t* idB,
                              uint8_t* type, uint32_t* ownerA, uint32_t* ownerB, uint8_t* side, float* force, float* torqueOnly,
                              float* cpA, float* cpB, size_t cap, size_t* nOut);
int deme_query_host_bytes(const deme_ctx* ctx, uint64_t* bytes);
/* Position code, orientation, velocity, angular velocity and family of a few owners, gathered on the device: row i of every
 * non-null column of `out` (columns of n entries) is owner ownerIds[i]'s value, bitwise what deme_download_owner_state gives at
 * that id.  Ids may repeat and come in any order; n == 0 is fine.  Refused (DEME_ERR_INVALID): an id out of range; a non-null a* /
 * alpha* column (those need the reduction a full download launches).  Read-only: no reduction is launched and the list, the
 * prescriptions and the step's buffers are left as they are.  64 bytes per id come to the host (added to deme_query_host_bytes). */
int deme_query_owner_state(deme_ctx* ctx, const uint32_t* ownerIds, size_t n, DemeOwnerState* out);
/* The counterpart: row i of every non-null column of `in` (columns of n entries) is written to owner ownerIds[i], on the device.
 * What is written is what deme_upload_owner_state writes for those columns -- position code, orientation, velocity, angular
 * velocity, and the family with the record's ghost / replicated bits kept --; every other field, the accumulators and every owner
 * not named keep their bits.  Ids come in any order.  Refused with nothing changed, no flag included (DEME_ERR_INVALID): a null
 * `in`; null ids with n > 0; an id out of range; an id given twice (the order of two writes is not defined); a non-null a* / alpha*
 * column (the caller does not take over the accumulators through this call: deme_upload_owner_state does that).  n == 0, or no
 * column at all, returns DEME_OK and changes nothing.  Otherwise the context's flags are set as deme_upload_owner_state sets them
 * for the same columns: the replayable step is dropped, the contact list is stale (any pose, velocity or family column: the next
 * step detects, also on a run with asynchronous detection), the prescriptions are looked up again (familyID).  There is no rule
 * that keeps the list when a write stays within the margins.  An error that is not one of these refusals (no memory for the
 * scratch, a failed copy) may leave the flags set, which costs a detection and nothing else.  Bytes: 68 * n go to the device (a 4-byte slot and a 64-byte record
 * per id), independent of the number of owners; they are added to deme_query_host_bytes. */
int deme_scatter_owner_state(deme_ctx* ctx, const uint32_t* ownerIds, size_t n, const DemeOwnerState* in);
/* The detection's radix sort alone, on host arrays (tests): a stable sort of keys (and vals with them) by the bits
 * [beginBit, endBit) of the key; the other bits take no part in the order and arrive unchanged.  forceOwn 1: the project's own
 * sort whatever n is (DEME_ERR_INVALID from a library built with rocprim at every site); 0: what the detection's call sites
 * take for a list of this kind and size -- rocprim below a threshold (pairs: keys of up to 20 bits count as crossing records,
 * wider ones as incidences).  deme_sort_tile_keys: the keys one workgroup of the own sort takes. */
int deme_sort_pairs_u32(int device, const uint32_t* keys, const uint32_t* vals, size_t n, unsigned beginBit, unsigned endBit, int forceOwn,
                        uint32_t* keysOut, uint32_t* valsOut);
int deme_sort_keys_u64(int device, const uint64_t* keys, size_t n, unsigned beginBit, unsigned endBit, int forceOwn, uint64_t* keysOut);
unsigned deme_sort_tile_keys(void);
/* The inspectors' segmented sum alone, on host arrays (tests): fp64 sums and counts by runs of equal keys, every addition in the
 * fixed order of deme_seg_sum.h.  keys: n ascending keys, the entries with a key >= nKeys (uncounted) behind the counted ones;
 * terms: n x lanes, row-major; sums: nKeys x lanes; counts: nKeys.  A key without a run gives zeros.  No sort inside.
 * Refused with DEME_ERR_INVALID: lanes other than an inspector's width (3, 4, 9, 11); n >= 2^31; a null array while n (keys,
 * terms) or nKeys (sums, counts) is not zero; keys that do not ascend. */
int deme_seg_sum_f64(int device, const uint32_t* keys, const double* terms, size_t n, unsigned lanes, uint32_t nKeys, double* sums,
                     uint32_t* counts);
/* per-sphere world position (LBF-shifted frame, as kT sees it) and inflated radius */
int deme_download_sphere_geometry(deme_ctx* ctx, double* X, double* Y, double* Z, float* R, size_t cap);

/* Resize clumps of a running simulation (DEMSolver::ChangeClumpSizes, API.h:1047): every sphere of owner ownerIds[i] (the caller's
 * numbering) gets relPos *= factors[i] and radius *= factors[i], one fp32 multiply of the current value each; repeated calls
 * compound.  Mass and moment of inertia are not changed (nor are they in the reference); owners without spheres are left alone.
 * The next step detects contacts with the new sizes; the history of pairs that stay in contact is kept.  Refused, with nothing
 * changed: an id out of range or given twice, a factor that is not finite or <= 0, a table of more than 65535 components.
 * Resized spheres get derived entries of the component table (shared by equal geometry); the first entries, the uploaded scene's,
 * always stay, derived entries no sphere uses any more are dropped. */
int deme_change_owner_sizes(deme_ctx* ctx, const uint32_t* ownerIds, const float* factors, size_t n);
int deme_num_components(const deme_ctx* ctx, uint32_t* n);
/* the component table in effect (deme_num_components entries; any pointer may be NULL) and every sphere's index into it, by the
 * caller's sphere id: what a scene re-upload needs to carry resized geometry over */
int deme_download_components(deme_ctx* ctx, float* relX, float* relY, float* relZ, float* radius, size_t cap);
int deme_download_sphere_components(deme_ctx* ctx, uint16_t* comp, size_t cap);
/* how many leading entries of the table are the scene's own (kept by every resize; the rest are derived and dropped when unused).
 * deme_upload_scene counts the whole uploaded table; a re-upload that carries derived entries over names the true count here. */
int deme_set_template_components(deme_ctx* ctx, uint32_t n);

/* Force-model hook (DEMForceModel::DefineCustomModel, AuxClasses.h:422-485;
 * equipForceModel APIPrivate.cpp:1381-1574): splice a user statement block into
 * the contact-force kernel and compile it for gfx950 at run time (hipRTC).
 * wildcardNames: nWildcards names of per-contact float history variables. */
int deme_compile_force_model(deme_ctx* ctx, const char* src, size_t len, const char* const* wildcardNames,
                             uint32_t nWildcards, const char* prerequisites);

/* Family motion prescriptions (SetFamilyPrescribedLinVel / AngVel / Position / Quaternion, AddFamilyPrescribedAcc /
 * AngAcc; API.h:720-838).  The three strings are the bodies of the `switch (family)` statements the reference generates in
 * equipFamilyPrescribedMotions (APIPrivate.cpp:1600-1708) for applyPrescribedVel / applyPrescribedPos /
 * applyAddedAcceleration (DEMIntegrationKernels.cu:8-98): "case <family>: { ...; break; }" sequences over the names
 * vX..omgBarZ, X, Y, Z, oriQw..oriQz, accX..angAccZ, t, ownerID and the ...Prescribed flags.  They are compiled for gfx950
 * with hipRTC; the families concerned must carry DEME_FAMILY_PRESCRIBED in DemeScene.familyFlags.  NULL / "" clears. */
int deme_compile_prescriptions(deme_ctx* ctx, const char* velCases, const char* posCases, const char* accCases);

/* On-the-fly family changes (DEMSolver::ChangeFamilyWhen, API.h:1024; kernel applyFamilyChanges,
 * DEMModeratorKernels.cu:10-60; run between the force evaluation and the integration of every step, dT.cpp:2437-2443).
 * `rules` is the _familyChangeRules_ text equipFamilyOnFlyChanges generates (APIPrivate.cpp:1576-1598).  If it mentions
 * acc / accX / accY / accZ the owners' contact accelerations are reduced before the rules run.  NULL / "" clears. */
int deme_compile_family_rules(deme_ctx* ctx, const char* rules);
/* DEMSolver::ChangeFamily(ID_from, ID_to) (API.h:1028): immediate, all owners of a family */
int deme_change_family(deme_ctx* ctx, uint32_t from, uint32_t to);

/* Adaptive controllers (reference: DEMKinematicThread::calibrateParams DEM/kT.cpp:43-98 -- bin-size
 * hill climb on kT's time per detection; DEMDynamicThread::calibrateParams DEM/dT.cpp:2276-2299 -- drift tuner;
 * API: UseAdaptiveBinSize, SetAdaptiveBinSizeDelaySteps / MaxRate / Acc / UpperProactivity / LowerProactivity,
 * UseAdaptiveUpdateFreq, SetCDMaxUpdateFreq, DEM/API.h:253-309).  Here both run on device timers (HIP events around the
 * detection / around a window of steps), inside deme_step:
 *  - bin size: every binObserveSteps detections the average device time per detection is compared with the previous
 *    window's; the change rate accelerates in the current direction on an improvement and turns round otherwise, with the
 *    reference's rule, clamps and safety overrides (too many spheres in a bin => shrink; too many bins => grow);
 *  - update frequency: this build has no second thread to drift ahead of, so the quantity tuned is K = cdUpdateFreq itself,
 *    hill-climbing the measured time per step (detection amortised over K + force pass over the K-inflated list) every
 *    freqObserveDetections detections, within [1, maxUpdateFreq].
 * Neither changes the physics: the contact set does not depend on the bin size, and a larger K only adds non-touching
 * pairs to the list (tests/test_adaptive.py: bit-identical state with the controllers on).  Off by default. */
typedef struct DemeAdaptive {
    uint32_t autoBinSize;           /* UseAdaptiveBinSize */
    uint32_t binObserveSteps;       /* SetAdaptiveBinSizeDelaySteps (reference default 25) */
    float binMaxRate;               /* SetAdaptiveBinSizeMaxRate (0.05) */
    float binAcc;                   /* SetAdaptiveBinSizeAcc (0.1) */
    float binUpperSafety;           /* 0.25: shrink when maxSpheresInBin > this * errOutBinSphNum */
    float binLowerSafety;           /* 0.3: grow when the bin count > this * 2^32 */
    uint32_t autoUpdateFreq;        /* UseAdaptiveUpdateFreq */
    uint32_t maxUpdateFreq;         /* SetCDMaxUpdateFreq */
    uint32_t freqObserveDetections; /* detections per adjustment of K */
} DemeAdaptive;
int deme_set_adaptive(deme_ctx* ctx, const DemeAdaptive* a);
/* current bin size / cdUpdateFreq and how many adjustments each controller has made */
int deme_get_adaptive_state(deme_ctx* ctx, double* binSize, uint32_t* cdUpdateFreq, uint32_t* nBinChanges, uint32_t* nFreqChanges);

/* Acceleration added by the script for the NEXT step only (reference: DEMTracker::AddAcc / AddAngAcc, AuxClasses.h:264-274 ->
 * DEMDynamicThread::addOwnerNextStepAcc / addOwnerNextStepAngAcc, dT.cpp:3160-3174: the values are written into a / alpha and a
 * flag keeps prepareAccArrays from clearing them once, DEMPrepForceKernels.cu:14-31 -- co-simulation hands forces over this way).
 * acc / angAcc: n x 3 floats for owners [owner, owner + n), either may be null; like the reference's setVal a second call
 * for the same owner replaces the first.  The integrator adds them to the contact sums of the coming step (after the sums,
 * whose order stays fixed) and the records clear themselves.  angAcc is in the owner's local frame like alpha. */
int deme_add_owner_acc(deme_ctx* ctx, uint32_t owner, uint32_t n, const float* acc, const float* angAcc);

/* Persistent contacts (reference: DEM/API.h:874-905 MarkFamilyPersistentContactEither/Both, MarkFamilyPersistentContact,
 * MarkPersistentContact and their Remove* inverses; DEM/APIPrivate.cpp:33-117; algorithms/DEMCubContactDetection.cu:605-802).
 * Qualifies contacts of the CURRENT list: mode 0 every contact, 1 either owner's family == N1, 2 both == N1, 3 the family
 * pair (N1, N2) in either order.  mark != 0: they stay in the contact list at every later detection whether or not the
 * sweep finds them (the force kernel still treats a separated pair as NOT_A_CONTACT); mark == 0: the qualification is
 * removed.  Refused for a history-less force model, like the reference.  Host-synchronous. */
int deme_mark_persistent_contacts(deme_ctx* ctx, int mode, uint32_t N1, uint32_t N2, int mark);
int deme_num_persistent_contacts(deme_ctx* ctx, size_t* n);
/* The marked set itself, as (sphere A, geometry B, contact type) triples in list order -- for a restart or a re-decomposition
 * (dem-engine_amd/decomp.py carries the marks to the ranks that own the pairs afterwards).  Upload replaces the set. */
int deme_download_persistent_contacts(deme_ctx* ctx, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap);
int deme_upload_persistent_contacts(deme_ctx* ctx, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, size_t n);

/* Owner and geometry wildcards of user force models (DEMForceModel::SetPerOwnerWildcards / SetPerGeometryWildcards,
 * AuxClasses.h:422-485; Models.h:319-360).  Owner wildcards are per-owner float arrays the fragment sees as `name`,
 * `name_A`, `name_B` (aliases, indexed by AOwner / BOwner); geometry wildcards are per-sphere / per-triangle /
 * per-analytical-component arrays seen as `name_A[AGeo]`, `name_B[BGeo]`.  Arrays start at zero; at most 8 of each.
 * deme_compile_force_model_ex declares them (after deme_upload_scene), the upload / download calls move one array:
 * kind 0 owners, 1 spheres, 2 triangles, 3 analytical components. */
int deme_compile_force_model_ex(deme_ctx* ctx, const char* src, size_t len, const char* const* contactWildcards, uint32_t nContactWc,
                                const char* const* ownerWildcards, uint32_t nOwnerWc, const char* const* geoWildcards,
                                uint32_t nGeoWc, const char* prerequisites);
int deme_upload_wildcard_array(deme_ctx* ctx, uint32_t kind, uint32_t index, const float* in, size_t n);
int deme_download_wildcard_array(deme_ctx* ctx, uint32_t kind, uint32_t index, float* out, size_t cap);

/* SetFamilyClumpMaterial / SetFamilyMeshMaterial (DEM/API.h:970-974; dT::setFamilyClumpMaterial, dT.cpp): every sphere
 * (kind 0) or triangle (kind 1) whose owner currently belongs to `family` takes material index `material` (load order, < nMat).
 * The per-contact records carry materials, so the next step starts with a contact detection. */
int deme_set_family_material(deme_ctx* ctx, uint32_t family, uint32_t material, int kind);
/* device memory in use / in total, as hipMemGetInfo reports it for the context's device (DEMSolver::ShowMemStats, API.h:584) */
int deme_device_memory(deme_ctx* ctx, size_t* usedBytes, size_t* totalBytes);

/* compile-only check of a fragment (no context, no GPU needed): same generator and hipRTC options,
 * 2 dummy materials; the compiler log is copied into `log`. */
int deme_jit_probe(const char* src, const char* const* wildcardNames, uint32_t nWildcards, const char* prerequisites,
                   char* log, size_t logCap);
/* the same with owner and geometry wildcards declared (DEMForceModel::SetPerOwnerWildcards / SetPerGeometryWildcards) */
int deme_jit_probe_ex(const char* src, const char* const* wildcardNames, uint32_t nWildcards, const char* const* ownerNames,
                      uint32_t nOwnerWc, const char* const* geoNames, uint32_t nGeoWc, const char* prerequisites, char* log,
                      size_t logCap);

/* Inspectors (DEMInspector, AuxClasses.cpp:19-170; kernels DEMSphereQueryKernels.cu:13-54,
 * DEMOwnerQueryKernels.cu:11-63; reduction dT.cpp:2556-2640): a per-sphere or per-owner quantity evaluated on
 * the device and reduced there.  Ghost owners of a slab decomposition are left out.  No region filter. */
#define DEME_INSPECT_CLUMP_MAX_Z 0          /* "clump_max_z": max over spheres of Z + radius */
#define DEME_INSPECT_CLUMP_MIN_Z 1          /* "clump_min_z" */
#define DEME_INSPECT_CLUMP_MAX_ABSV 2       /* "clump_max_absv": sphere-centre speed incl. rotation */
#define DEME_INSPECT_CLUMP_MASS 3           /* "clump_mass": sum over clump owners */
#define DEME_INSPECT_MAX_ABSV 4             /* "max_absv": max owner speed, all owner kinds */
#define DEME_INSPECT_CLUMP_KINETIC_ENERGY 5 /* "clump_kinetic_energy" */
#define DEME_INSPECT_ABSV 6                 /* "absv": per-owner values only (deme_inspect_values) */
#define DEME_INSPECT_CLUMP_VOLUME 7         /* "clump_volume": sum of the declared template volumes (deme_upload_volumes) */
int deme_inspect(deme_ctx* ctx, uint32_t quantity, float* out);
/* unreduced values (DEMInspector::GetValues): one per sphere (quantities 0-2) or per owner (3-6) */
int deme_inspect_values(deme_ctx* ctx, uint32_t quantity, float* out, size_t cap);
/* Region-limited inspection (reference: DEMSolver::CreateInspector(quantity, region) DEM/API.h:675, AuxClasses.cpp:205-223).
 * `code` is the reference's region string: a C++ statement block that returns a bool from float X, Y, Z (sphere centre for
 * the per-sphere quantities, owner CoM otherwise), e.g. "return (X * X + Y * Y <= 0.25 * 0.25) && (Z <= -0.3);".  It is
 * compiled once at run time; elements outside the region do not take part in the reduction (an empty region yields the
 * reduction's identity: -FLT_MAX / FLT_MAX / 0).  deme_inspect(q) == deme_inspect_region(q, -1). */
int deme_compile_region(deme_ctx* ctx, const char* code, int* regionId);
int deme_inspect_region(deme_ctx* ctx, uint32_t quantity, int regionId, float* out);
/* Declared clump volumes, one per mass-property entry (reference: DEMClumpTemplate::volume, APIPrivate.cpp:730, 1849-1858). */
int deme_upload_volumes(deme_ctx* ctx, const float* volumes, size_t n);
/* Contact inspectors (no counterpart in the reference): the virial sum and the coordination of a bed, summed over the current
 * contact list on the device.  The rows are those deme_download_contact_records gives.
 *   A row is COUNTED when, in fp64, (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)forceThreshold^2, f the recorded force
 *   (record 0; the torque-only force takes no part).
 *   A SIDE of a counted row is counted when its owner is a clump owner of this context, is no ghost copy and lies in the region
 *   -- the owner's centre of mass tested as deme_inspect_region tests it for the per-owner quantities; regionId -1: everywhere.
 *   Mesh and analytical owners are never counted sides.  Side A carries +f and cpA, side B -f and cpB.
 *   A counted side adds the outer product virial[3 * i + j] += r_i * f_j, r = R(q) cp, q the owner's stored quaternion as it stands
 *   (not renormalised), R(q)v = v + 2w(u x v) + 2u x (u x v) with u = (qx, qy, qz); cp and q converted to fp64 first, everything
 *   computed in fp64.  The Love-Weber stress of a region of volume V is virial / V (the caller divides); compression is negative.
 * sides: the counted sides; clumps: the own, non-ghost clump owners in the region, with or without contacts -- the mean
 * coordination number is sides / clumps.  The sum has a fixed order: two calls on the same state give the same bits.
 * deme_inspect_contact_counts: the counted sides per owner in the caller's numbering (nOwners entries; 0 for owners that are no
 * clumps or lie outside the region).
 * Read-only: no reduction of the step is launched; the list, the prescriptions and the step's buffers stay as they are.  Only the
 * result comes to the host: sizeof(DemeContactSums) = 88 bytes, or 4 bytes per owner; both are added to deme_query_host_bytes.
 * Refused with DEME_ERR_INVALID and nothing written: a null output; an unknown region; cap < nOwners; a threshold that is negative
 * or not finite; recording off or a seeded list (the messages of deme_download_contact_records). */
typedef struct DemeContactSums {
    double virial[9]; /* row-major */
    uint64_t sides;
    uint64_t clumps;
} DemeContactSums;
int deme_inspect_contacts(deme_ctx* ctx, int regionId, float forceThreshold, DemeContactSums* out);
int deme_inspect_contact_counts(deme_ctx* ctx, int regionId, float forceThreshold, uint32_t* perOwner, size_t cap);
/* Contact loads per mesh triangle (no counterpart in the reference): which faces carry the load, summed over the current contact
 * list on the device.  The rows are those deme_download_contacts / deme_download_contact_records give.
 *   A row is COUNTED when it is a sphere-mesh row (DEME_SPHERE_MESH_CONTACT) whose B is a triangle id < nTri, the owner of sphere
 *   A is no ghost copy (a slab of a decomposed run), and (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)forceThreshold^2,
 *   f the recorded force (record 0; the torque-only force takes no part) -- the test deme_inspect_contacts makes.  With a threshold
 *   of 0 every such row of the list counts, rows with zero force included.
 *   A counted row adds -f to its triangle -- the force ON the triangle, in the world frame; deme_inspect_contacts gives side B the
 *   same sign -- and 1 to the triangle's count.  The force sum is fp64 over the fp32 records.  A triangle without a counted row
 *   gets zeros.
 * The order of every floating-point addition is fixed by the list and the grid (no floating-point atomics): two calls on the same
 * state give the same bits.
 * force: 3 doubles per asked triangle; contacts: one count per asked triangle; either may be NULL.  Only the asked range
 * [firstTri, firstTri + nTris) comes to the host: 24 + 4 bytes per asked triangle for the columns asked for, added to
 * deme_query_host_bytes.  nTris == 0 returns DEME_OK and launches nothing.
 * Read-only: no reduction of the step is launched; the list, the prescriptions and the step's buffers stay as they are.
 * Refused with DEME_ERR_INVALID and nothing written: a threshold that is negative or not finite; a range beyond the scene's
 * triangles; both outputs NULL while nTris > 0; recording off or a seeded list (as deme_download_contact_records).
 * deme_tri_loads_block_rows: the sorted rows one workgroup of the segmented sum takes (a triangle with more rows than that is
 * summed by several workgroups). */
int deme_inspect_tri_loads(deme_ctx* ctx, float forceThreshold, uint32_t firstTri, uint32_t nTris, double* force /* 3 per triangle, or NULL */,
                           uint32_t* contacts /* 1 per triangle, or NULL */);
unsigned deme_tri_loads_block_rows(void);
/* Mesh wear (no counterpart in the reference): contact impulse and sliding work per mesh triangle, summed over the samples of a run
 * on the device -- the time integrals deme_inspect_tri_loads gives one instant of; Archard's law is V = k/H * INT |Fn| |v_slide| dt.
 * The accumulators live on the device from sample to sample: a sample costs device passes only, no read-back and no host wait, and
 * the numbers come to the host when deme_tri_wear_read asks.  Everything below is fp64 over the fp32 values as stored.
 *   WHICH ROWS COUNT.  The rows are those deme_download_contacts / deme_download_contact_records give.  A row is COUNTED exactly as
 *   deme_inspect_tri_loads counts it: its class is sphere-mesh (DEME_SPHERE_MESH_CONTACT); B is a triangle id < nTri; sphere A is <
 *   nSpheres and A's owner is a valid slot and no ghost copy; (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)forceThreshold^2,
 *   f the recorded force (record 0).
 *   QUANTITIES OF A COUNTED ROW.  oA: the owner of sphere A; oB: the owner of triangle B.  R(q)v = v + 2w(u x v) + 2u x (u x v), u =
 *   (qx, qy, qz): the rotation of deme_inspect_contacts, with the stored quaternion as it stands (not renormalised).
 *     rA = R(qA) cpA, rB = R(qB) cpB                     (records 2 and 3)
 *     wA = R(qA) (omgBarX, omgBarY, omgBarZ)_A, wB alike (the stored angular velocity is in the body frame)
 *     vA = v_A + wA x rA, vB = v_B + wB x rB
 *     u  = vA - vB            the velocity of the sphere's contact point relative to the face's
 *     g  = -f                 the force ON the triangle, the sign of deme_inspect_tri_loads
 *     N  = R(qB) ((n2 - n1) x (n3 - n1))   from the triangle's owner-local nodes as they stand (deme_update_tri_nodes may have moved them)
 *     if N.N > 0:  nh = N / sqrt(N.N), Fn = g.nh, gt = g - Fn nh, ut = u - (u.nh) nh;  otherwise (a degenerate face) lanes 3 to 5 add 0
 *   THE SIX LANES of a sample of weight w (seconds), each w times:
 *     0..2  g_x, g_y, g_z     N s   the impulse on the face
 *     3     |Fn|              N s   the normal impulse
 *     4     |Fn| * |ut|       J     the Archard sliding work: normal load times sliding distance
 *     5     |gt| * |ut|       J     the shear work
 *   and a counted row adds 1 to the triangle's rows, a uint64_t.
 *   WHICH STATE A SAMPLE PAIRS.  The state as it stands: the records of the last force pass with the owners' CURRENT records (velocity,
 *   angular velocity, orientation) and the triangles' current nodes -- as deme_inspect_contacts pairs the records with the current
 *   quaternion.  After deme_step(n) that is the force at the start of the last step with the state at its end.
 *   ORDER OF ADDITIONS.  Within a triangle and a sample the terms are added in list order down the fixed tree of the segmented sum;
 *   the sample's sum is then added once to the accumulator, by the one thread that finishes that triangle.  No floating-point
 *   atomics: two runs of the same sequence of steps and samples give the same bits.
 * deme_tri_wear_enable(on != 0) allocates and clears 56 bytes a triangle; enabling twice keeps the sums; on == 0 frees them.  It needs
 * an uploaded scene; a scene without triangles is fine, and every call then does nothing.  A deme_upload_scene that changes nTri clears
 * the accumulators and the sampled time at the new size; one that keeps nTri keeps them.
 * deme_tri_wear_sample adds one sample and returns once its passes are enqueued on the context's stream, behind the steps already
 * there: no host wait, and no bytes counted by deme_query_host_bytes.  Refused with DEME_ERR_INVALID and nothing changed, in this
 * order: not enabled; a threshold that is negative or not finite; a weight that is negative or not finite; recording off (the
 * message of deme_download_contact_records).  A list whose contacts have NOT BEEN EVALUATED is no error: a seeded list
 * (deme_seed_contacts, or the engine's order was just renewed), or a list that was just put in force -- by deme_detect_contacts, or by
 * an asynchronous detection (deme_set_async_detection) whose cycle ended with the last deme_step call -- while the records in memory
 * are still those of the list before it.  The call then returns DEME_OK with *sampled = 0 and adds nothing; the caller carries the
 * weight to its next sample.  Otherwise *sampled = 1 and the sampled time grows by the weight, also when the list or the mesh is
 * empty.  sampled may be NULL.  A weight of 0 counts rows and adds zeros.
 * deme_tri_wear_read waits for the stream and copies only the asked range [firstTri, firstTri + nTris) and the asked columns (any
 * may be NULL): 24 / 8 / 8 / 8 / 8 bytes per asked triangle for impulse / normalImpulse / slidingWork / shearWork / rows, all added
 * to deme_query_host_bytes.  sampledTime (one number: the sum of the weights since the last clear) comes from the host's own sum.
 * nTris == 0 launches nothing.  Refused: not enabled; a range beyond the scene's triangles; every output NULL while nTris > 0.
 * deme_tri_wear_reset clears the accumulators and the sampled time.
 * Nothing the step reads is written: the list, the prescriptions and the step's buffers stay as they are, with an asynchronous
 * detection too.  Event timers (deme_kernel_time_ms): "tri_wear_select", "tri_wear_sort", "tri_wear_sums". */
int deme_tri_wear_enable(deme_ctx* ctx, int on);
int deme_tri_wear_sample(deme_ctx* ctx, float forceThreshold, double weight, int* sampled /* or NULL */);
int deme_tri_wear_read(deme_ctx* ctx, uint32_t firstTri, uint32_t nTris, double* impulse /* 3 per triangle */, double* normalImpulse,
                       double* slidingWork, double* shearWork, uint64_t* rows, double* sampledTime /* one number: the sum of the weights */);
int deme_tri_wear_reset(deme_ctx* ctx);
/* Field inspector (no counterpart in the reference): per-cell sums on a regular grid -- what solid fraction, mean velocity, granular
 * temperature, contact stress and coordination are derived from, cell by cell -- summed on the device.
 *   GRID.  nCells = n[0] * n[1] * n[2]; the id of cell (ix, iy, iz) is ix + n[0] * (iy + n[1] * iz); every per-cell array is in that
 *   order.
 *   CELL OF AN OWNER.  P_k is the owner's centre of mass in the world frame in fp64, decoded as the run-time compiled kernels decode
 *   it (decode_pos(...)_k + (double)LBF_k).  u_k = (P_k - origin[k]) / cell[k] in fp64, no contraction.  The owner is inside iff
 *   u_k >= 0.0 && u_k < (double)n[k] on all three axes (a NaN is outside); i_k = (uint32_t)u_k.  So a cell's lower face belongs to
 *   it, its upper face to the next cell, and the grid's upper faces to nobody.
 *   A COUNTED OWNER is an own clump owner -- its caller id is < nOwnerClumps, the test deme_inspect_contacts makes -- that is no
 *   ghost copy and lies inside the grid.  Fixed and prescribed families count like any clump; mesh and analytical owners never do.
 *   OWNER COLUMNS of a cell: sums over its counted owners, every term converted to fp64 first and computed as written:
 *     clumps    uint32_t   1
 *     mass      double     (double)m, m the mass of the owner's mass-property entry
 *     volume    double     (double)volume of that entry, as declared with deme_upload_volumes
 *     momentum  3 doubles  (double)m * (double)v_k
 *     kinetic   6 doubles  xx, yy, zz, xy, xz, yz: ((double)m * (double)v_i) * (double)v_j
 *   CONTACT COLUMNS of a cell.  A row is COUNTED by the test of deme_inspect_contacts: record 0, the squared fp32 components summed
 *   in fp64 and compared >= (double)forceThreshold^2.  A SIDE of a counted row belongs to the cell of its owner, if that owner is a
 *   counted owner -- the cell of the owner's centre of mass, not of the contact point: the per-particle Love-Weber average
 *   sigma = (1 / V) sum_p sum_c r (x) f.
 *     sides     uint32_t   1 per counted side
 *     virial    9 doubles  row-major, the r_i * f_j deme_inspect_contacts adds for the side: r = R(q) cp with the stored quaternion;
 *                          side A carries +f and cpA, side B -f and cpB
 *   DERIVED, by the caller, with V = cell[0] * cell[1] * cell[2]: solid fraction volume / V; mean velocity momentum / mass; kinetic
 *   stress -(kinetic - p (x) p / mass) / V; granular temperature trace(kinetic - p (x) p / mass) / (3 mass); contact stress
 *   virial / V; coordination sides / clumps.
 *   ORDER.  Within a cell the terms are added in a fixed order -- owner slots ascending; sides in list order, A before B -- down a
 *   tree of fixed shape: two calls on one state give the same bits.  No floating-point atomics; no workgroup waits for another.
 * Any column may be NULL; only the asked columns come to the host: 4, 8, 24, 48 or 72 bytes per cell, added to
 * deme_query_host_bytes.  The caller's arrays are written once the call can no longer fail.  Owner columns alone need no contact
 * records.  Read-only: the list, the prescriptions and the step's buffers stay as they are.
 * Refused with DEME_ERR_INVALID and nothing written, in this order: a null grid or null columns; an origin or cell edge that is not
 * finite; a cell edge <= 0; an n[k] == 0; nCells > 2^21; every column NULL; a threshold that is negative or not finite; volume asked
 * without uploaded volumes; sides or virial asked with recording off or a seeded list (as deme_download_contact_records); a list of
 * 2^31 rows or more.
 * deme_fields_block_rows: the sorted entries one workgroup of the segmented sums takes. */
typedef struct DemeFieldGrid {
    double origin[3]; /* world frame: lower corner of cell (0, 0, 0) */
    double cell[3];   /* edge lengths */
    uint32_t n[3];    /* cells along x, y, z */
} DemeFieldGrid;
typedef struct DemeFieldColumns { /* any may be NULL; nCells entries (times 3 / 6 / 9) each */
    uint32_t* clumps;
    double* mass;
    double* volume;
    double* momentum;
    double* kinetic;
    uint32_t* sides;
    double* virial;
} DemeFieldColumns;
#define DEME_FIELDS_MAX_CELLS (1u << 21)
int deme_inspect_fields(deme_ctx* ctx, const DemeFieldGrid* grid, float forceThreshold, const DemeFieldColumns* out);
unsigned deme_fields_block_rows(void);
/* Cluster inspector (no counterpart in the reference, whose GetClumpContacts hands the pairs to the script): the connected components
 * of the contact network, labelled on the device -- how many agglomerates or fragments there are, how large and heavy each is, where
 * its centre lies, which clumps are rattlers outside the force network.
 *   VERTICES.  A vertex is an own clump owner -- its caller id is < nOwnerClumps, the test deme_inspect_contacts makes -- that is no
 *   ghost copy.  In a slab of a decomposed run the ghost copies of clumps are vertices too, for linking only: they are never counted.
 *   Mesh and analytical owners are never vertices, so a floor does not join the bed into one cluster.
 *   EDGES.  An edge is a row of the current list of class sphere-sphere that is counted by the test of deme_inspect_contacts --
 *   record 0, (double)fx^2 + (double)fy^2 + (double)fz^2 >= (double)forceThreshold^2 -- whose two spheres belong to two DIFFERENT
 *   owners that are both vertices.  With a threshold of 0 every such listed row is an edge, rows with zero force included.
 *   LABEL.  The label of a vertex is the smallest caller owner id of its connected component: a pure function of the graph, whatever
 *   the order the threads ran in.  An owner that is no vertex gets 0xFFFFFFFF.
 *   SUMMARY.  vertices; edges: the counted rows that are edges (several rows between one pair of clumps count each); clusters;
 *   singletons: the clusters of size 1; largestSize; largestLabel: the smallest label among the clusters of the largest size
 *   (0xFFFFFFFF when there is no vertex).
 *   CLUSTER TABLE.  One row per cluster that has at least one COUNTED owner -- an own clump that is no ghost copy --, labels
 *   ascending:
 *     label    uint32_t
 *     size     uint32_t   the cluster's counted owners
 *     mass     double     the sum of (double)m, m the mass of the owner's mass-property entry
 *     moment   3 doubles  the sum of (double)m * P_k, P the owner's centre of mass in the world frame in fp64, decoded as
 *                         deme_inspect_fields decodes it (decode_pos(...)_k + (double)LBF_k); the cluster's centre is moment / mass
 *                         (the caller divides)
 *   ORDER.  Within a cluster the terms are added owner slots ascending, down a tree of fixed shape; the integers are summed with
 *   integer atomics or on a fixed grid: two calls on one state give the same bits.  No floating-point atomics.
 * Any output may be NULL, and any column of the table.  *nClusters always receives the table's row count (also when table is NULL,
 * and when the call returns for too small a tableCap); with tableCap < *nClusters no row is written and the call returns
 * DEME_ERR_INVALID: ask with table NULL, size the arrays, ask again -- the protocol of deme_query_owner_contacts.  The caller's
 * arrays are written once the call can no longer fail.
 * Bytes that come to the host, all added to deme_query_host_bytes: 16 for the row count and the control words of every call that
 * is not refused; 48 for the summary; 4 per owner for the labels; 4 + 4 + 8 + 24 per table row for the asked columns.
 * Read-only: the list, the prescriptions and the step's buffers stay as they are.
 * Refused with DEME_ERR_INVALID and nothing written (nClusters neither, no byte added), in this order: every output NULL; labels
 * given with labelCap < nOwners; a threshold that is negative or not finite; recording off or a seeded list (the messages of
 * deme_download_contact_records); a list of 2^31 rows or more.
 * No loop on the device is unbounded: a find takes at most nOwners steps, a link at most nOwners retries; a bound that is passed
 * sets a flag, and the call returns DEME_ERR_INTERNAL with nothing written.
 * deme_clusters_link_retries: the compare-and-swaps the link pass of the last call lost to another thread (a measurement). */
typedef struct DemeClusterSummary {
    uint64_t vertices;
    uint64_t edges;
    uint64_t clusters;
    uint64_t singletons;
    uint64_t largestSize;
    uint64_t largestLabel;
} DemeClusterSummary;
typedef struct DemeClusterColumns { /* any may be NULL; tableCap entries (times 3) each */
    uint32_t* label;
    uint32_t* size;
    double* mass;
    double* moment;
} DemeClusterColumns;
int deme_inspect_clusters(deme_ctx* ctx, float forceThreshold, DemeClusterSummary* summary, uint32_t* labels, size_t labelCap,
                          const DemeClusterColumns* table, size_t tableCap, size_t* nClusters);
int deme_clusters_link_retries(const deme_ctx* ctx, uint64_t* retries);

/* timing of the kernels this library launched (HIP events on the context stream);
 * names: "calc_forces", "integrate", "detect", the passes of deme_inspect_tri_loads "tri_loads_select", "tri_loads_sort",
 * "tri_loads_sums", and those of deme_inspect_fields "fields_cells" (both select kernels), "fields_sort", "fields_sums", and those of deme_inspect_clusters
 * "clusters_label" (init, link, flatten, summary), "clusters_sort" (select, scan, sort), "clusters_sums"; returns avg ms per launch
 * since last reset */
int deme_kernel_time_ms(deme_ctx* ctx, const char* name, double* avg_ms, uint64_t* launches);
int deme_kernel_time_reset(deme_ctx* ctx);
/* enable = 0: off; n > 0: every n-th launch of each timed kernel is bracketed with events (an event pair costs ~3 us of
 * dispatch gap, 4.7 % of a 0.29 ms step when every launch is timed) */
int deme_set_timing(deme_ctx* ctx, int enable);

/* multi-GPU slab decomposition helpers (no reference equivalent).
 * pack/unpack ghost-owner state into a caller-provided DEVICE buffer that the
 * host exchanges with RCCL send/recv. 56 bytes per ghost. */
#define DEME_GHOST_BYTES 56
int deme_halo_pack(deme_ctx* ctx, const uint32_t* d_ownerIDs, uint32_t n, void* d_buf);
int deme_halo_unpack(deme_ctx* ctx, const uint32_t* d_ownerIDs, uint32_t n, const void* d_buf);

/* Halo exchange overlapped with the interior force evaluation (north_star; no reference equivalent).  The context owns a
 * second stream for the ghost traffic.  Per step:
 *   deme_step_overlap_begin   forces of the owner runs that read no ghost owner (compute stream); *detectionDue = 1 when
 *                             this step starts with a contact detection, which needs the ghosts first: nothing is launched
 *   deme_halo_pack_async      pack on the halo stream, ordered after the previous step's integration
 *   (the caller's send / recv of the packed records, enqueued on deme_halo_stream)
 *   deme_halo_unpack_async    unpack on the halo stream
 *   deme_step_overlap_end     compute stream waits for the unpack; remaining forces, integration
 *                             (or, when a detection was due, the whole un-split step)
 * The two force passes together evaluate every contact exactly once, in the same arithmetic as deme_step. */
int deme_halo_stream(deme_ctx* ctx, void** hipStream);
int deme_halo_pack_async(deme_ctx* ctx, const uint32_t* d_ownerIDs, uint32_t n, void* d_buf);
int deme_halo_unpack_async(deme_ctx* ctx, const uint32_t* d_ownerIDs, uint32_t n, const void* d_buf);
int deme_halo_sync(deme_ctx* ctx);
int deme_step_overlap_begin(deme_ctx* ctx, int* detectionDue);
int deme_step_overlap_end(deme_ctx* ctx);


/* ---- the exchange driven from the library (north_star: "RCCL halo exchange of ghost clumps over xGMI ... overlapped with
 * interior force evaluation on a second HIP stream", host orchestration in C++).  A halo group = one RCCL communicator + the
 * slabs this process holds (normally one: one process per GPU; several slabs in one process exchange by sends to self, which is
 * how the path is tested on a single GPU).  RCCL is bound at run time (a process with PyTorch loaded shares PyTorch's copy).
 *   deme_halo_unique_id       ncclGetUniqueId: rank 0 calls it and hands the 128 bytes to the other ranks (any side channel)
 *   deme_halo_group_create    ncclCommInitRank(world, id, rank) on `device`; id == NULL with world == 1: a one-rank communicator
 *   deme_halo_group_attach    a slab: its context, and per side the neighbour's rank (-1: none; the own rank together with the
 *                             neighbour's context when this process holds it), the LOCAL owner ids whose records are sent there
 *                             and the local owner ids (ghost copies) that take the records arriving from there; lists in the
 *                             same clump order on both sides (dem-engine_amd/decomp.py builds them)
 *   deme_halo_group_step      nsteps x { interior force pass | pack -> ncclGroupStart, ncclSend / ncclRecv per face,
 *                             ncclGroupEnd -> unpack | ghost-dependent force pass, [ncclAllReduce of the replicated free
 *                             owners' a / alpha,] integration } for every attached slab; asynchronous like deme_step
 *                             (deme_halo_group_sync waits)
 *   deme_halo_group_exchange  the exchange alone (ghost copies refreshed after an upload) */
typedef struct deme_halo_group deme_halo_group;
int deme_halo_unique_id(unsigned char* id128);
int deme_halo_group_create(const unsigned char* id128, int rank, int world, int device, deme_halo_group** out);
void deme_halo_group_destroy(deme_halo_group* g);
const char* deme_halo_group_last_error(const deme_halo_group* g);
int deme_halo_group_attach(deme_halo_group* g, deme_ctx* ctx, int leftRank, deme_ctx* leftLocal, const uint32_t* sendLeft,
                           uint32_t nSendLeft, const uint32_t* recvLeft, uint32_t nRecvLeft, int rightRank, deme_ctx* rightLocal,
                           const uint32_t* sendRight, uint32_t nSendRight, const uint32_t* recvRight, uint32_t nRecvRight);
int deme_halo_group_step(deme_halo_group* g, uint32_t nsteps);
int deme_halo_group_exchange(deme_halo_group* g);
int deme_halo_group_sync(deme_halo_group* g);
int deme_halo_group_stats(const deme_halo_group* g, uint64_t* exchanges, uint64_t* bytesSentPerStep);
/* host microseconds spent enqueuing since creation / the last reset: [0] interior force passes, [1] packs, [2] the RCCL group,
 * [3] unpacks + boundary passes + integration */
int deme_halo_group_host_time(deme_halo_group* g, double us[4], int reset);
/* Migration inside the library (SURVEY 8e "migration at re-bin time"; the algorithm of decomp.migrate_neighbours, on the device).
 *   deme_halo_group_set_slab     what the group has to know about a slab beyond its exchange lists: global clump / sphere ids of
 *                                its owners and spheres (scene order: own clumps, ghosts from the left, ghosts from the right,
 *                                replicated owners), the slab's x range [xLo, xHi) and the halo thickness; flipMask: the contact
 *                                wildcards that are B->A vectors (bit w; 7 = delta_tan_x/y/z of the Hertzian model)
 *   deme_halo_group_migrate      collective over the group: every own clump whose centre crossed a face moves to that face
 *                                neighbour with its state, template ids and the history rows of its contacts (global sphere
 *                                ids; ncclSend / ncclRecv between ranks, buffer hand-over between slabs of one process), ghost
 *                                sets are renewed from the neighbours' current clumps, every slab is re-assembled and re-seeded on
 *                                the device and its exchange lists rebuilt.  Only counts pass through the host.  The next step of
 *                                every slab starts with a contact detection.
 *   deme_halo_group_slab_counts  own / ghost-left / ghost-right clumps, owners, spheres, seeded contacts of a slab
 *   deme_halo_group_download_ids global ids (and sphere -> owner / component) of a slab's current numbering, for the caller's books */
int deme_halo_group_set_slab(deme_halo_group* g, deme_ctx* ctx, const uint32_t* ownerGlobal, const uint32_t* sphereGlobal, uint32_t nOwn,
                             uint32_t nGhostLeft, uint32_t nGhostRight, double xLo, double xHi, double halo, uint32_t flipMask);
int deme_halo_group_migrate(deme_halo_group* g, uint32_t* clumpsMoved);
int deme_halo_group_slab_counts(const deme_halo_group* g, const deme_ctx* ctx, uint32_t counts[6]);
int deme_halo_group_download_ids(deme_halo_group* g, deme_ctx* ctx, uint32_t* ownerGlobal, uint32_t* sphereGlobal, uint32_t* sphereOwner,
                                 uint16_t* sphereComp);
/* how many ranks the group's RCCL communicator spans, as RCCL itself reports it (ncclCommCount): a scaling run checks this
 * against the number of processes it believes it launched */
int deme_halo_group_comm_count(const deme_halo_group* g, int* ranks);
/* One evaluation -- and one contact history -- per contact that straddles a cut (the reference's rule that a pair
 * belongs to exactly one bin, DEMContactKernels_SphereSphere.cu:212, carried over to ranks).  0 (default): both ranks evaluate a
 * contact between an own clump and a ghost, each keeps its history copy, the force on the ghost is dropped.  1: the LEFT slab of a
 * cut evaluates it; the right slab leaves the pair (and its ghosts' wall / mesh contacts) off its list, and after the
 * ghost-dependent force pass of every step the left slab sends a / alpha of each right ghost's contact sum to the ghost's owner
 * (32 bytes per ghost, ncclSend / ncclRecv in one group, the forward exchange's lists read backwards), which adds them before
 * integrating.  Call after every slab is attached; the contact lists are rebuilt at the next step.  Not combined with replicated
 * free owners (DemeScene.ownerGhost = 2). */
int deme_halo_group_set_cross_contacts(deme_halo_group* g, int evaluateOnce);

/* ---- the decomposition itself, behind the C-ABI (round 5; north_star: "the reference's two-GPU kT/dT split is replaced by a per-GPU
 * spatial-domain decomposition ... host orchestration in C++").  The reference picks its devices in the constructor
 * (DEM/API.h:52-56, DEM/APIPublic.cpp:22-110: DEMSolver(nGPUs) / DEMSolver(device ids)); here that constructor opens a deme_multi.
 *
 * deme_decomp_*: the PLAN -- pure host code, no device needed.  A global scene (no ghosts) is cut into nSlabs slabs along `axis`
 * (0 / 1 / 2, or -1: the longest side of the clumps' bounding box) at equal-count boundaries snapped to bin faces (`edges`: nSlabs + 1
 * boundaries of the caller's own instead; the outer two are taken as -inf / +inf); a slab's scene is [own clumps | ghosts from the
 * lower neighbour | ghosts from the upper neighbour | replicated owners], a ghost being a neighbour's clump whose centre lies within
 * `halo` of the shared face (halo <= 0: four clump reaches + twice the widest family margin).  Every rule is the one
 * dem-engine_amd/decomp.py states in numpy (the CPU tests hold the two against each other). */
#define DEME_DECOMP_SHARED_FREE 1u /* allow replicated owners that move under contact forces (DemeScene.ownerGhost = 2) */
#define DEME_DECOMP_NO_SNAP 2u     /* keep the equal-count boundaries where the quantiles put them (not snapped to bin faces) */
#define DEME_DECOMP_SPATIAL_ORDER 4u /* number every slab's own clumps in the engine's own order (compact owner tiles, csrc/deme_order.inc;
                                      * ghosts follow their owner slab's order) instead of by ascending global id: a scene with ghosts keeps
                                      * the order it is uploaded in, so this is what gives a slab of a sampler-ordered bed its tiles.
                                      * deme_multi_build sets it unless DEME_DECOMP_CALLER_ORDER is given */
#define DEME_DECOMP_CALLER_ORDER 8u
typedef struct deme_decomp deme_decomp;
int deme_decomp_create(const DemeParams* p, const DemeScene* scene, uint32_t nSlabs, int axis, double halo, const double* edges, uint32_t flags,
                       deme_decomp** out, char* err, size_t errCap);
void deme_decomp_destroy(deme_decomp* d);
int deme_decomp_info(const deme_decomp* d, uint32_t* nSlabs, int* axis, double* halo, double* edges /* nSlabs + 1 */, uint32_t* nFreeReplicated);
/* one slab of the plan: its scene (pointers into the plan's storage: valid until deme_decomp_destroy), {own, ghosts from below, ghosts
 * from above} clump counts, the global owner id of every slab owner and the global sphere id of every slab sphere, the LOCAL owner
 * ids sent to the lower / upper neighbour (what arrives lands on the ghost ranges, in order), the slab's range along the axis */
int deme_decomp_slab(const deme_decomp* d, uint32_t slab, DemeScene* scene, uint32_t counts[3], const uint32_t** ownerGlobal,
                     const uint32_t** sphereGlobal, const uint32_t** sendLower, uint32_t* nSendLower, const uint32_t** sendUpper,
                     uint32_t* nSendUpper, double range[2]);

/* The slabs of a plan that THIS rank holds (slab s belongs to rank s * world / nSlabs; nSlabs must be a multiple of the group's world)
 * become contexts on the group's device: deme_ctx_create, deme_set_arith_mode(arith: DEME_ARITH_*, or -1 for the process default),
 * deme_set_params, deme_upload_scene, deme_halo_group_attach, deme_halo_group_set_slab (flipMask as there), then one exchange.
 * The contexts belong to the group (deme_halo_group_destroy destroys them); deme_halo_group_slab_ctx hands them out in slab order
 * for what a script sets per context (force models, prescriptions, recording ...).  deme_halo_group_set_axis: the axis the slabs of
 * an attach-by-hand group were cut along (default 0; _build sets it from the plan). */
int deme_halo_group_build(deme_halo_group* g, const DemeParams* p, const deme_decomp* plan, int arith, uint32_t flipMask);
int deme_halo_group_set_axis(deme_halo_group* g, int axis);
int deme_halo_group_slab_ctx(deme_halo_group* g, uint32_t i, deme_ctx** ctx, uint32_t* globalSlab);
int deme_halo_group_num_slabs(const deme_halo_group* g, uint32_t* n);
/* Owner state by GLOBAL owner id: every slab of this rank writes its OWN clumps' rows (replicated owners: the first slab's) into the
 * caller's arrays of the global scene's length / reads them from there (ghost copies are refreshed by one exchange).  With several
 * ranks each process fills / takes only its part. */
int deme_halo_group_download_state(deme_halo_group* g, DemeOwnerState* global, uint32_t nOwnersGlobal);
int deme_halo_group_upload_state(deme_halo_group* g, const DemeOwnerState* global, uint32_t nOwnersGlobal);

/* One process, several devices: the reference's DEMSolver(nGPUs) / DEMSolver(std::vector<int>) (DEM/API.h:52-56).  deme_multi_create
 * checks every id against the visible devices (an absent one: DEME_ERR_INVALID, the message names it -- GpuManager.cpp:64-68 throws
 * there), opens one halo group per device -- one RCCL rank each, the communicators initialised together in one grouped
 * ncclCommInitRank -- and deme_multi_build cuts the scene into nDevices * slabsPerDevice slabs (deme_decomp_create) and hands every
 * device its block (deme_halo_group_build).  deme_multi_step steps all groups (one host thread per device when there are several:
 * each group's loop is the per-process loop of deme_halo_group_step) and migrates clumps between slabs every `migrateEvery` steps
 * (deme_multi_set_migration; 0 = never).  With one device and one slab per device this is a plain context behind the same calls. */
typedef struct deme_multi deme_multi;
int deme_multi_create(const int* devices, int nDevices, deme_multi** out, char* err, size_t errCap);
void deme_multi_destroy(deme_multi* m);
const char* deme_multi_last_error(const deme_multi* m);
int deme_multi_build(deme_multi* m, const DemeParams* p, const DemeScene* scene, uint32_t slabsPerDevice, int axis, double halo, uint32_t flags,
                     int arith, uint32_t flipMask);
int deme_multi_num_slabs(const deme_multi* m, uint32_t* n);
int deme_multi_slab_ctx(deme_multi* m, uint32_t slab, deme_ctx** ctx);
/* the same handle for questions that change nothing (kernel names, bin size, timers): the merged contact list of the run stays valid */
int deme_multi_slab_ctx_peek(const deme_multi* m, uint32_t slab, const deme_ctx** ctx);
int deme_multi_set_migration(deme_multi* m, uint32_t migrateEvery);
int deme_multi_step(deme_multi* m, uint32_t nsteps);
int deme_multi_sync(deme_multi* m);
int deme_multi_download_state(deme_multi* m, DemeOwnerState* global, uint32_t nOwnersGlobal);
int deme_multi_upload_state(deme_multi* m, const DemeOwnerState* global, uint32_t nOwnersGlobal);
/* contacts of all slabs together (a contact that straddles a cut is on two lists unless deme_halo_group_set_cross_contacts(1):
 * `nContacts` counts list entries), steps taken, detections of the first slab, clumps that changed slabs so far */
int deme_multi_counts(deme_multi* m, DemeCounts* sum, uint64_t* clumpsMigrated);
/* back to the state after deme_multi_create (slabs, contexts and plan dropped; the groups opened anew): a scene re-upload */
int deme_multi_reset(deme_multi* m);
/* The contact list of a decomposed run in GLOBAL sphere ids (analytical-component / triangle ids are global already): a pair that
 * straddles a cut is reported once, sphere-sphere pairs as (smaller, larger) id, rows in the canonical order of an undivided
 * context (A, then class, then B).  Per-contact wildcards and recorded forces / contact points follow in the same order; where a slab
 * held a pair the other way round, its B -> A vector wildcards (the flipMask given at build) and its recorded force change sign and
 * its two contact points swap.  The list is rebuilt after every step / state upload. */
/* deme_change_owner_sizes by GLOBAL owner id: every slab resizes its own clumps and its ghost copies; one table, planned from all
 * slabs' keys, goes to every slab.  DEME_ERR_HALO, with nothing changed, when the largest clump would reach more than half the
 * halo the plan was cut with (build the run again with a wider halo). */
int deme_multi_change_owner_sizes(deme_multi* m, const uint32_t* globalIds, const float* factors, size_t n);
int deme_multi_download_sphere_components(deme_multi* m, uint16_t* comp, size_t cap); /* by global sphere id */
int deme_multi_num_contacts(deme_multi* m, size_t* n);
int deme_multi_download_contacts(deme_multi* m, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap);
int deme_multi_download_contact_wildcard(deme_multi* m, uint32_t w, float* out, size_t cap);
int deme_multi_download_contact_records(deme_multi* m, float* force, float* torqueOnly, float* cpA, float* cpB, size_t cap);
/* deme_query_owner_contacts for a decomposed run, in GLOBAL ids: every slab selects from its own list on its device, with the rule
 * of the merged list (a pair reported once, by the slab that owns the clump of the globally smaller sphere; a pair the slab holds
 * the other way round flipped: force and torque-only force times -1, contact points swapped), and the host sorts the hits of all
 * slabs by the merged key.  The answer is the sub-sequence of deme_multi_download_contacts / deme_multi_download_contact_records
 * whose rows touch one of ownerIds, bit for bit, in that list's order; ownerA / ownerB are global owner ids, side as above in the
 * merged orientation.  A repeated id counts once; *nOut receives the hit count and with cap < *nOut no row is written
 * (DEME_ERR_INVALID).  Refused with nothing written (nOut included): an id >= the global owner count; withRecords while recording
 * is off on a slab or a slab's list is a seed, as in the step after a migration (the messages of
 * deme_multi_download_contact_records).  The call waits for the run (deme_multi_sync); it neither uses nor invalidates the merged
 * list, downloads no slab's list and none of its id books.  The scratch belongs to the slabs' contexts and is kept between calls.
 * deme_multi_query_host_bytes: every byte these calls and deme_multi_query_owner_state have copied from a device to the host since
 * deme_multi_create -- 4 per slab and selection pass (the hit count; a slab whose hits exceed its scratch selects twice, a slab
 * with an empty list not at all), 24 per hit row, 48 more per hit row with records; for the state call 4 per slab and 64 per owner
 * found on it. */
int deme_multi_query_owner_contacts(deme_multi* m, const uint32_t* ownerIds, size_t nOwners, int withRecords, uint32_t* idA, uint32_t* idB,
                                    uint8_t* type, uint32_t* ownerA, uint32_t* ownerB, uint8_t* side, float* force, float* torqueOnly,
                                    float* cpA, float* cpB, size_t cap, size_t* nOut);
int deme_multi_query_host_bytes(const deme_multi* m, uint64_t* bytes);
/* deme_query_owner_state by GLOBAL owner id: every slab gathers the listed owners it answers for (its own clumps; the replicated
 * owners on the first slab of the chain -- the rule of deme_multi_download_state) on its device.  Values equal
 * deme_multi_download_state indexed by the ids, bit for bit. */
int deme_multi_query_owner_state(deme_multi* m, const uint32_t* globalIds, size_t n, DemeOwnerState* out);
/* deme_scatter_owner_state by GLOBAL owner id, with its refusals.  Every copy takes the value: the clump in the slab that owns
 * it, its ghost copies in the neighbour slabs, a replicated owner on every slab -- as deme_multi_upload_state writes them; the state
 * afterwards equals that upload's, bit for bit.  A position written across a cut moves no clump between slabs before the next
 * migration, as with the whole upload.  The flags are set on every slab and the merged list is dropped.  An error that is not a
 * refusal may leave the slabs before the failing one written.  The call waits for the
 * run (deme_multi_sync).  Bytes: 68 * n per slab go to the devices (the sorted ids and their records; every slab searches them for
 * the owners it holds), independent of the number of owners; added to deme_multi_query_host_bytes. */
int deme_multi_scatter_owner_state(deme_multi* m, const uint32_t* globalIds, size_t n, const DemeOwnerState* in);
/* Restart and marked pairs of a decomposed run, in GLOBAL ids: deme_seed_contacts / deme_*_persistent_contacts for every slab that holds
 * a pair (both geometries present, one of them the slab's own), in the slab's ids and with the slab's sign of the B -> A vector
 * wildcards; the downloads report a pair once (sphere-sphere pairs smaller id first, ascending). */
int deme_multi_seed_contacts(deme_multi* m, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, const float* wildcards, size_t n);
int deme_multi_mark_persistent_contacts(deme_multi* m, int mode, uint32_t N1, uint32_t N2, int mark);
int deme_multi_num_persistent_contacts(deme_multi* m, size_t* n);
int deme_multi_download_persistent_contacts(deme_multi* m, uint32_t* idA, uint32_t* idB, uint8_t* type, size_t cap);
int deme_multi_upload_persistent_contacts(deme_multi* m, const uint32_t* idA, const uint32_t* idB, const uint8_t* type, size_t n);
/* deme_upload_contact_wildcard for the merged list (n = deme_multi_num_contacts): every slab's copy of a pair takes the value */
int deme_multi_upload_contact_wildcard(deme_multi* m, uint32_t w, const float* in, size_t n);
/* Moving the slab boundaries: equal counts again from the clumps' CURRENT coordinates (snapped to bin faces), then the migration of
 * deme_halo_group_migrate moves the clumps that now lie beyond a boundary.  One call moves a boundary by less than the narrower of its
 * two slabs minus the halo (a clump travels to a face neighbour only); newEdges (nSlabs + 1, may be NULL) receives the boundaries in
 * force afterwards.  deme_multi_slab_counts: {own, ghosts below, ghosts above, owners, spheres, seeded contacts} and the range of a slab. */
int deme_multi_rebalance(deme_multi* m, uint32_t* clumpsMoved, double* newEdges);
/* every n-th migration that deme_multi_step finds due (deme_multi_set_migration) recomputes the boundaries first; 0: never (default) */
int deme_multi_set_rebalance(deme_multi* m, uint32_t everyNthMigration);
int deme_multi_slab_counts(deme_multi* m, uint32_t slab, uint32_t counts[6], double range[2]);
/* deme_download / _upload_wildcard_array by GLOBAL id (kind 0: per owner, 1: per sphere; n = the global scene's count): a row is read
 * from the slab that owns the clump (a replicated owner's from the first slab) and written to every copy.  Kinds 2, 3 (triangles,
 * analytical components: replicated geometry) are written to every slab and read back from the first one.  The library's
 * migration carries owner and sphere wildcard arrays with the clumps (deme_halo_group_migrate). */
int deme_multi_download_wildcard_array(deme_multi* m, uint32_t kind, uint32_t index, float* out, size_t cap);
int deme_multi_upload_wildcard_array(deme_multi* m, uint32_t kind, uint32_t index, const float* in, size_t n);
/* deme_inspect_values by GLOBAL id (per sphere for the sphere-wise quantities, per owner otherwise) */
int deme_multi_inspect_values(deme_multi* m, uint32_t quantity, float* out, size_t cap);
/* deme_inspect_contacts / deme_inspect_contact_counts for a decomposed run.  Every slab answers over its OWN clumps on its device
 * (ghost sides are left out, as by every inspector): a contact across a cut gives its A side on one slab and its B side on the
 * other, each from that slab's own record and the owner's current pose.  The host adds the slabs' results in slab order (fp64 for
 * virial, integers for the rest); the per-owner counts are indexed by GLOBAL owner id (cap >= the global owner count) through the
 * slabs' device books.  regionCode: a region string as deme_compile_region takes it, compiled once per slab context and kept by
 * its text; NULL or blank: everywhere.  The call waits for the run (deme_multi_sync).  Refused as the single-context calls are --
 * a slab without recording, or whose list is a seed as in the step after a migration, with the messages of
 * deme_multi_download_contact_records -- and while the run evaluates every cross-cut contact once
 * (deme_halo_group_set_cross_contacts): the slab that does not evaluate a pair holds no record of it.  Bytes, added to
 * deme_multi_query_host_bytes: 88 per slab, or 4 per global owner and slab. */
int deme_multi_inspect_contacts(deme_multi* m, const char* regionCode /* NULL or blank: everywhere */, float forceThreshold, DemeContactSums* out);
int deme_multi_inspect_contact_counts(deme_multi* m, const char* regionCode, float forceThreshold, uint32_t* perOwnerGlobal, size_t cap);
/* deme_inspect_tri_loads for a decomposed run.  Triangles carry the same ids on every slab; every slab sums its own list on its
 * device, and since a row whose sphere belongs to a ghost copy is not counted, each sphere-triangle pair is counted by exactly one
 * slab.  The host adds the slabs' arrays in slab order.  The call waits for the run (deme_multi_sync).  Refused as the single-context
 * call is (a slab without recording, or whose list is a seed).  A run that evaluates every cross-cut contact once
 * (deme_halo_group_set_cross_contacts) would be refused too; no call of this interface puts a deme_multi into that mode today, so
 * that refusal cannot be met yet.  Bytes, added to deme_multi_query_host_bytes: 24 + 4 per asked triangle and slab. */
int deme_multi_inspect_tri_loads(deme_multi* m, float forceThreshold, uint32_t firstTri, uint32_t nTris, double* force, uint32_t* contacts);
/* deme_tri_wear_* for a decomposed run.  Every slab samples its own list on its own device into its own accumulators; since a row
 * whose sphere belongs to a ghost copy is not counted, a pair is counted by the one slab that owns sphere A's clump.  A sample is all
 * or nothing: if any slab's list is a seed -- the step after a migration -- no slab adds anything and *sampled = 0.  It waits for
 * nothing.  _read waits for the run and adds the slabs' arrays in slab order; bytes per slab and asked triangle as
 * deme_tri_wear_read, added to deme_multi_query_host_bytes.  The refusals of the single-context calls; _enable(on), _sample and _read
 * are refused too while the run evaluates every cross-cut contact once (deme_halo_group_set_cross_contacts): the slab that does not
 * evaluate a pair holds no record of it. */
int deme_multi_tri_wear_enable(deme_multi* m, int on);
int deme_multi_tri_wear_sample(deme_multi* m, float forceThreshold, double weight, int* sampled);
int deme_multi_tri_wear_read(deme_multi* m, uint32_t firstTri, uint32_t nTris, double* impulse, double* normalImpulse, double* slidingWork,
                             double* shearWork, uint64_t* rows, double* sampledTime);
int deme_multi_tri_wear_reset(deme_multi* m);
/* deme_inspect_fields for a decomposed run.  Every slab sums over its OWN clumps on its device (a clump is an own clump of one slab
 * only, ghost copies never count); all slabs' passes are enqueued first, then the host takes the asked columns slab by slab and adds
 * them in slab order: the asked columns' bytes per cell and slab, added to deme_multi_query_host_bytes.  The refusals of
 * deme_inspect_fields; when a contact column is asked also those of deme_multi_inspect_contacts (a run that evaluates every cross-cut
 * contact once; a slab whose list is a seed, as on the step after a migration). */
int deme_multi_inspect_fields(deme_multi* m, const DemeFieldGrid* grid, float forceThreshold, const DemeFieldColumns* out);
/* deme_inspect_clusters for a decomposed run: the same outputs in GLOBAL owner ids (labelCap counts global owners).  Every slab
 * labels its own clumps and its ghost copies in its local ids and hands down, per local owner, the pair (global id, global id of
 * its local root), and its table keyed by the local root and summed over its OWN clumps only (a clump is an own clump of one slab).
 * The host unites the pairs in one array union-find with the same smaller-id-wins rule; the label is the root of the global id.  The
 * slabs' table rows are added into their final label in slab order, within a slab local roots ascending: a fixed order.  An edge
 * is counted by the slab that owns the clump with the smaller global id; the rest of the summary is computed from the merged table.
 * The call waits for the run.  The refusals of deme_inspect_clusters' arguments, then those of deme_multi_inspect_contacts (a run
 * that evaluates every cross-cut contact once; a slab without recording, or whose list is a seed as on the step after a migration).
 * Bytes per slab, added to deme_multi_query_host_bytes: 16 + 48, 8 per local owner, 40 per row of the slab's table. */
int deme_multi_inspect_clusters(deme_multi* m, float forceThreshold, DemeClusterSummary* summary, uint32_t* labels, size_t labelCap,
                                const DemeClusterColumns* table, size_t tableCap, size_t* nClusters);
/* deme_add_owner_acc by GLOBAL owner id: a clump's entry goes to the slab that owns it, a replicated owner's to every slab */
int deme_multi_add_owner_acc(deme_multi* m, uint32_t owner, uint32_t n, const float* acc, const float* angAcc);
/* the visible HIP devices (0 and DEME_OK where there is none: what the constructors check ids against) */
int deme_device_count(int* n);
/* Measurement aid (quote the attainable rate beside the nominal 8 TB/s): a hand-written 16 B / lane streaming copy of
 * `bytes` (choose well beyond the 256 MiB Infinity Cache), best of `reps` timings, read + written bytes per second in GB/s. */
int deme_copy_rate_probe(int device, size_t bytes, int reps, double* GBs);
/* {owners, clump owners, spheres, contact wildcards} of the scene a context holds (a slab's change when clumps migrate) */
int deme_scene_sizes(const deme_ctx* ctx, uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* DEME_HIP_H */
