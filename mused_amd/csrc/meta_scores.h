// Scores of the two-column metadata records (/root/reference/matrix_operations.py:22-54, 250-263), shared by
// meta.hip (score matrices) and knn.hip (selection straight from the records).
#pragma once
#include <hip/hip_runtime.h>

namespace mused {

// Every operation is rounded on its own (no fused multiply-add), in the order the reference's Python expression
// evaluates it, so that the only difference to the host arithmetic is the last-bit accuracy of sin / cos / asin.  The
// operators are written out under the function's own `fp contract(off)`: __dmul_rn, __dsub_rn and __dadd_rn do not do here --
// the header's inline bodies are compiled under the default contraction mode and fuse once inlined (lat2d * d2r - lat1 as
// one v_fma_f64 is the rounding error of the product, not 0, for two equal latitudes).
__device__ __forceinline__ double haversine_km(double lat1d, double lon1d, double lat2d, double lon2d) {
#pragma clang fp contract(off)
  const double d2r = 3.14159265358979323846 / 180.0;  // math.radians: x * (pi / 180)
  const double lat1 = lat1d * d2r, lon1 = lon1d * d2r;
  const double lat2 = lat2d * d2r, lon2 = lon2d * d2r;
  const double dlat = lat2 - lat1, dlon = lon2 - lon1;
  const double sdlat = sin(dlat * 0.5);
  const double sdlon = sin(dlon * 0.5);
  const double cc = cos(lat1) * cos(lat2);
  const double sq_lat = sdlat * sdlat, sq_lon = sdlon * sdlon;
  const double t = cc * sq_lon;
  const double a = sq_lat + t;
  const double c = 2.0 * asin(sqrt(a));
  return c * 6371.0;
}

// |datetaken_j - datetaken_i| + |dateupload_j - dateupload_i| (:40-50)
__device__ __forceinline__ double time_l1(double a0, double a1, double b0, double b1) {
#pragma clang fp contract(off)
  return __dadd_rn(fabs(__dsub_rn(b0, a0)), fabs(__dsub_rn(b1, a1)));
}

}  // namespace mused
