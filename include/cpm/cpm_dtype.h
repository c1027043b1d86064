/* cpm_dtype.h -- what the library and its hosts both need to know about a cpm_dtype (cpm.h, which includes this header): whether a code
 * is one, and the bytes of a voxel.  Header-only: no symbol is exported and CPM_ABI_VERSION is untouched.  Constant expressions in C++,
 * where the device-side trait (csrc/cpm_voxel.h) is checked against them at compile time. */
#ifndef CPM_CPM_DTYPE_H
#define CPM_CPM_DTYPE_H
#include "cpm.h"
#ifdef __cplusplus
#define CPM_DTYPE_FN constexpr
#else
#define CPM_DTYPE_FN static inline
#endif

CPM_DTYPE_FN int cpm_dtype_valid(int32_t dtype) { return dtype >= CPM_U8 && dtype <= CPM_I16; }
/* bytes per voxel (4 for anything but the 1- and 2-byte types: an invalid code is refused where a volume is described) */
CPM_DTYPE_FN size_t cpm_dtype_size(int32_t dtype) { return dtype == CPM_U8 ? 1 : (dtype == CPM_U16 || dtype == CPM_F16 || dtype == CPM_I16 ? 2 : 4); }

#undef CPM_DTYPE_FN
#endif /* CPM_CPM_DTYPE_H */
