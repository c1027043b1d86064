// cpm_voxel.h -- the voxel types' one home in the library (DESIGN.md "Adding a voxel type"): what a cpm_dtype (include/cpm/cpm.h) means
// to the host code that describes a volume, the device-side trait that reads one voxel, and the switch that turns a runtime dtype
// into a kernel instantiation.  Validity and element size are the public cpm_dtype_valid / cpm_dtype_size (include/cpm/cpm_dtype.h).
#pragma once
#include "cpm/cpm.h"
#include "cpm_math.hip.h"

namespace cpm {

// ---- host side
// the raw values a type spans -- what a difference brick's mean |b - a| is divided by (float types and I16's w(v): 1) ...
inline double dtype_range(int dtype) { return dtype == CPM_U8 ? 255.0 : (dtype == CPM_U16 ? 65535.0 : 1.0); }
// ... and the factor that takes a widened voxel to [0, 1]: 1 / 255, 1 / 65535, 1 (one f32 division of exact operands)
inline float dtype_norm(int dtype) { return 1.0f / (float)dtype_range(dtype); }
// cpm_volume_desc_default's pair.  I16 (SNORM): [-1, 1] -> [0, 1], as Inviwo maps signed normalised formats; every other type is used as it is
inline float dtype_default_offset(int dtype) { return dtype == CPM_I16 ? 1.0f : 0.0f; }
inline float dtype_default_scaling(int dtype) { return dtype == CPM_I16 ? 0.5f : 0.0f; }
// a kernel's view of the value mapping (v * norm + offset) * one_minus_scaling: tracer::VolDev and the brick kernels' BrickVol
template <typename V> void set_value_mapping(V& v, const cpm_volume_desc& d) {
    v.norm = dtype_norm(d.dtype); v.offset = d.format_offset; v.one_minus_scaling = 1.0f - d.format_scaling;
}

// ---- device side
// Voxel<DT>: the storage type T of one voxel, its size, whether it is a float type (one that can hold NaN and inf), and widen(), the
// f32 value every consumer works on: the integer itself (u8, u16), the exact widening (binary16), w(v) of cpm.h (int16).  The 1- and
// 2-byte types take the voxel zero-extended to a word: what a T converts to, and what a shift and mask leave of a loaded word.
template <typename S, bool FLOAT> struct VoxelStorage {
    typedef S T;
    static constexpr int size = (int)sizeof(S);
    static constexpr bool is_float = FLOAT;
};
template <int DT> struct Voxel;
template <> struct Voxel<CPM_U8> : VoxelStorage<uint8_t, false> { static CPM_DEV float widen(uint32_t t) { return (float)t; } };
template <> struct Voxel<CPM_U16> : VoxelStorage<uint16_t, false> { static CPM_DEV float widen(uint32_t t) { return (float)t; } };
template <> struct Voxel<CPM_F32> : VoxelStorage<float, true> { static CPM_DEV float widen(float t) { return t; } };
template <> struct Voxel<CPM_F16> : VoxelStorage<uint16_t, true> { static CPM_DEV float widen(uint32_t t) { return half_to_float(t); } };
template <> struct Voxel<CPM_I16> : VoxelStorage<uint16_t, false> { static CPM_DEV float widen(uint32_t t) { return snorm16_to_float(t); } };
static_assert(Voxel<CPM_U8>::size == cpm_dtype_size(CPM_U8) && Voxel<CPM_U16>::size == cpm_dtype_size(CPM_U16) &&
              Voxel<CPM_F32>::size == cpm_dtype_size(CPM_F32) && Voxel<CPM_F16>::size == cpm_dtype_size(CPM_F16) &&
              Voxel<CPM_I16>::size == cpm_dtype_size(CPM_I16), "Voxel<>::T and cpm_dtype_size disagree");

// ---- dispatch
// Runs M(CPM_<type>) for the runtime `dtype`; M pastes its argument into a kernel's template arguments.  A macro, not a generic
// lambda: CPM_LAUNCH (cpm_ctx.h) turns its kernel argument into the name the profiling hook reports, and that name spells the
// enumerator (trace_kernel<CPM_U8, ...>).  default: a volume's dtype was checked by cpm_volume_create, so it is F32.
#define CPM_DISPATCH_DTYPE(dtype, M)        \
    do { switch (dtype) {                   \
        case CPM_U8: M(CPM_U8); break;      \
        case CPM_U16: M(CPM_U16); break;    \
        case CPM_F16: M(CPM_F16); break;    \
        case CPM_I16: M(CPM_I16); break;    \
        default: M(CPM_F32); break;         \
    } } while (0)
// The narrower sibling for a kernel that is instantiated for some types only (the brick row kernels of cpm_correlated.hip): the
// caller has turned every other type away and names the three that are left -- A, B and REST, which takes whatever else arrives.
#define CPM_DISPATCH_DTYPE3(dtype, M, A, B, REST) \
    do { switch (dtype) { case A: M(A); break; case B: M(B); break; default: M(REST); break; } } while (0)

}  // namespace cpm
