// Lock-free union-find over a device array parent[] (parent[x] <= x always: the larger root is hooked under the smaller, so a
// tree's root is its smallest member).  Shared by dbscan.hip (core-core edges) and emst.hip (Boruvka picks).  Every access
// is a device-scope vector atomic on global memory; no caller waits for another.
#pragma once
#include "common.h"

namespace mused {

__device__ __forceinline__ int db_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; halves the path on its way (a row that has a parent below itself is never a root again, and any ancestor is a
// valid parent: the stores race with nothing that matters)
__device__ __forceinline__ int db_find(int* parent, int x) {
  int p = db_load(parent + x);
  while (p != x) {
    const int g = db_load(parent + p);
    if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = g;
  }
  return x;
}

// joins the trees of a and b; returns the smaller of the two roots it ended with.  joined (optional): whether THIS call's
// compare-and-swap hooked one root under the other (false: the two were, or became through someone else, one tree)
__device__ __forceinline__ int db_unite(int* parent, int a, int b, bool* joined = nullptr) {
  if (joined) *joined = false;
  while (true) {
    a = db_find(parent, a);
    b = db_find(parent, b);
    if (a == b) return a;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) {
      if (joined) *joined = true;
      return lo;
    }
    a = old;  // hi was hooked elsewhere in the meantime: on from its new parent
    b = lo;
  }
}

}  // namespace mused
