/*
 * vggsfm_amd -- device self-tests (libvggsfm_amd_selftest.so, a library of its own: the entries of libvggsfm_amd.so and the
 * headers under include/ are a closed, counted set).  Entries that run the shared __device__ helpers of csrc/ on a caller's
 * data and hand every lane's result back, so that a test can compare them with a restatement of its own.
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous, no allocation,
 * VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggs_; their rows stand in vggsfm_amd/_lib_selftest.py.
 */
#ifndef VGGSFM_AMD_SELFTEST_H
#define VGGSFM_AMD_SELFTEST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* rows of `out` of vggs_crosslane */
#define VGGS_GROUP_SUM_8 0
#define VGGS_GROUP_SUM_16 1
#define VGGS_GROUP_SUM_32 2
#define VGGS_GROUP_SUM_64 3
#define VGGS_WAVE_SUM 4
#define VGGS_WAVE_MAX 5
#define VGGS_WAVE_BCAST 6
#define VGGS_NUM_PRIMS 7

const char* vggs_build_arch(void);

/* Every cross-lane primitive of csrc/crosslane.hpp, applied to one value per lane.  num_blocks workgroups of 256 threads;
 * thread t of workgroup b is element e = 256 b + t of `in` (num_blocks x 256 doubles) and of every row of `out`
 * (VGGS_NUM_PRIMS x num_blocks x 256 doubles): out[r][e] = what primitive r returned in that lane.
 *
 * skip (num_blocks x 4 uint64, may be NULL = all zero): one word per wavefront, bit i standing for lane i.  The aligned group
 * of W lanes whose FIRST lane's bit is set does not call group_sum<W> -- it branches around the call, so the call runs with a
 * partial EXEC mask -- and leaves its elements of that row of `out` as they were.  The rows of the primitives that need the
 * whole wavefront (VGGS_GROUP_SUM_64 and above, and the reduce-scatter) are written only by wavefronts whose word is 0.
 *
 * VGGS_WAVE_BCAST broadcasts lane bcast_src (0 .. 63) of each wavefront.
 *
 * scatter_in (num_blocks x 256 x scatter_values doubles, element-major; may be NULL): scatter_values values per lane, summed
 * over each wavefront by the reduce-scatter butterfly into scatter_out (num_blocks x 4 x scatter_values).  scatter_values is
 * one of 6, 14, 24, 28, 36, 45 (the counts the camera pass uses). */
int vggs_crosslane(const double* in, const uint64_t* skip, int num_blocks, int bcast_src, const double* scatter_in,
                   int scatter_values, double* out, double* scatter_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
