// deme_owner_cols.h -- the columns of DemeOwnerState (include/deme_hip.h), listed once, in the struct's order.
//
// DEME_OWNER_COLS(P, A, F) calls one macro per column with (ABI field, element type, device record, field of that record):
//   P  a pose or velocity column: OwnerRec, written by owner id too (deme_scatter_owner_state)
//   A  an accumulator column (a / alpha): AccRec, moved only by a whole upload or download
//   F  familyID: a pose column whose word shares OwnerRec::family with the flag bits, so whoever moves it writes its line by
//      hand: (r.family & OWNER_FLAG_BITS) | value on a write, (uint8_t)r.family on a read
// A user that treats columns alike passes one macro several times; DEME_COL_NONE skips a kind.  Generated from the list: OwnerSoA
// and k_pack_owners (deme_kernels.h), the scatter bits and scatter_state_write (deme_query.h), the owner_state_* helpers of
// deme_hip.hip, OwnerStateBuf and group_state_io (deme_decomp.inc).  Not one of the headers embedded for run-time compilation.
#pragma once
#include "../../include/deme_hip.h"
#include "deme_device.h"

#define DEME_OWNER_COLS(P, A, F)            \
    P(voxelID, uint64_t, OwnerRec, voxelID) \
    P(locX, uint16_t, OwnerRec, locX)       \
    P(locY, uint16_t, OwnerRec, locY)       \
    P(locZ, uint16_t, OwnerRec, locZ)       \
    P(oriQw, float, OwnerRec, qw)           \
    P(oriQx, float, OwnerRec, qx)           \
    P(oriQy, float, OwnerRec, qy)           \
    P(oriQz, float, OwnerRec, qz)           \
    P(vX, float, OwnerRec, vx)              \
    P(vY, float, OwnerRec, vy)              \
    P(vZ, float, OwnerRec, vz)              \
    P(omgBarX, float, OwnerRec, wx)         \
    P(omgBarY, float, OwnerRec, wy)         \
    P(omgBarZ, float, OwnerRec, wz)         \
    A(aX, float, AccRec, ax)                \
    A(aY, float, AccRec, ay)                \
    A(aZ, float, AccRec, az)                \
    A(alphaX, float, AccRec, lx)            \
    A(alphaY, float, AccRec, ly)            \
    A(alphaZ, float, AccRec, lz)            \
    F(familyID, uint8_t, OwnerRec, family)
#define DEME_COL_NONE(abi, T, Rec, f)

namespace deme_dev {

// the scatter mask: bit k = pose column k (the accumulator columns take no bit)
enum : uint32_t {
#define DEME_COL_IX(abi, T, Rec, f) DEME_POSE_IX_##abi,
    DEME_OWNER_COLS(DEME_COL_IX, DEME_COL_NONE, DEME_COL_IX)
#undef DEME_COL_IX
    DEME_N_POSE_COLS
};
#define DEME_SCATTER_BIT(abi) (1u << DEME_POSE_IX_##abi)
static_assert(DEME_SCATTER_BIT(voxelID) == 0x0001u && DEME_SCATTER_BIT(locX) == 0x0002u && DEME_SCATTER_BIT(locY) == 0x0004u &&
                  DEME_SCATTER_BIT(locZ) == 0x0008u && DEME_SCATTER_BIT(oriQw) == 0x0010u && DEME_SCATTER_BIT(oriQx) == 0x0020u &&
                  DEME_SCATTER_BIT(oriQy) == 0x0040u && DEME_SCATTER_BIT(oriQz) == 0x0080u && DEME_SCATTER_BIT(vX) == 0x0100u &&
                  DEME_SCATTER_BIT(vY) == 0x0200u && DEME_SCATTER_BIT(vZ) == 0x0400u && DEME_SCATTER_BIT(omgBarX) == 0x0800u &&
                  DEME_SCATTER_BIT(omgBarY) == 0x1000u && DEME_SCATTER_BIT(omgBarZ) == 0x2000u && DEME_SCATTER_BIT(familyID) == 0x4000u &&
                  DEME_N_POSE_COLS == 15,
              "the scatter bits are 0x0001 ... 0x4000 in the order of DemeOwnerState");

#define DEME_COL_CHECK(abi, T, Rec, f)                                                                                     \
    static_assert(sizeof(T) == sizeof(*DemeOwnerState{}.abi), #abi ": element size against DemeOwnerState");               \
    static_assert(sizeof(T) == sizeof(Rec{}.f), #abi ": element size against " #Rec "::" #f);
#define DEME_COL_CHECK_F(abi, T, Rec, f) /* one byte of the 32-bit family word */ \
    static_assert(sizeof(T) == sizeof(*DemeOwnerState{}.abi) && sizeof(T) == 1 && sizeof(Rec{}.f) == 4, #abi ": element size");
DEME_OWNER_COLS(DEME_COL_CHECK, DEME_COL_CHECK, DEME_COL_CHECK_F)
#undef DEME_COL_CHECK
#undef DEME_COL_CHECK_F

}  // namespace deme_dev
