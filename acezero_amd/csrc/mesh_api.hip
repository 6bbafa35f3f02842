// mesh_api.hip -- the connected components of a triangle mesh and the mesh without its small ones (include/acez.h section P:
// acez_mesh_components, acez_mesh_component_counts, acez_mesh_select, acez_mesh_compact). clean_mesh.py, fuse_depth.py
// --min_component_faces / --min_component_ratio / --keep_largest.
//
// The header's section P is the definition; tests/mesh_restated.py restates it in numpy. Everything here is integer arithmetic: the
// labels, the counts and the compacted mesh are functions of the mesh alone, whatever the schedule.
//
// components  a lock-free union-find over the vertices, three launches: init (parent[v] = v), hook, flatten. d_labels is parent[].
//   hook      one lane per face unites (a, b) and (b, c): find both roots, CAS the LARGER root under the SMALLER, retry from the new
//             roots when the CAS fails. parent[v] <= v at all times and only ever decreases, so a walk strictly descends, a vertex is
//             linked at most once (the CAS expects parent[hi] == hi, and a vertex with a smaller parent never gets itself back), the
//             smallest vertex of a component can never get a parent, and the last root standing is that smallest vertex. The walk
//             halves its path (parent[v] <- min(parent[v], grandparent), an atomic min, so the invariants hold): without it a strip
//             whose vertices ascend builds one chain of m links and every find walks it.
//             Every access to parent[] in this launch is a relaxed AGENT-scope atomic: the workgroups of one launch run on eight
//             XCDs with private L2s, a plain load may be served from a line that another XCD's CAS has long replaced, and a find
//             that walks such lines can hand the CAS a stale root for ever.
//   flatten   after the kernel boundary plain loads and stores do: label[v] = root of v, in place. A lane that meets a label another
//             lane has already flattened reads a root or an older ancestor; both lead to the same root, which no lane changes.
//   Both loops are capped at m + 1 trips and report an overrun in *d_status instead of spinning; the comments at the loops say why
//   the cap cannot be reached. No lane ever waits for another: a failed CAS means that another lane's CAS succeeded.
// counts      integer atomic adds by label. One component usually holds nearly every face, so where the active lanes of a wavefront
//             share a label one lane adds their number once; otherwise every lane adds its own 1.
// select      flag mode: which faces stay, which vertices they use (plain byte stores of 1).
// compact     scatter mode: with the inclusive sums of those flags (the caller's torch.cumsum), the kept rows move to their new places.
// Every index formed from device data (a face's vertices, a label, a rank) is range-checked before it is used as an address: wrong
// tables give wrong numbers, never an access out of bounds.
#include <stdint.h>

#include "acez_common.h"
#include "launch1d.h"

namespace {

using namespace acez;

constexpr int MS_THREADS = 256;

#define MS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// a, b, c of face t and whether it is valid: every index in 0 .. m - 1, no two equal
__device__ __forceinline__ bool load_face(const int32_t* __restrict__ faces, int64_t t, int m, int& a, int& b, int& c) {
  a = faces[3 * t];
  b = faces[3 * t + 1];
  c = faces[3 * t + 2];
  return a >= 0 && a < m && b >= 0 && b < m && c >= 0 && c < m && a != b && b != c && a != c;
}

__global__ void __launch_bounds__(MS_THREADS) init_kernel(int32_t* __restrict__ parent, int m) {
  const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (v < m) parent[v] = (int32_t)v;
}

// The root of v's tree at some moment of the walk. Every step goes to a strictly smaller vertex (parent[x] < x unless x is a root),
// so there are fewer than m of them: the cap of m + 1 cannot be reached unless parent[] holds something this launch never wrote.
__device__ __forceinline__ int find_root(int32_t* parent, int v, int m, int32_t* status) {
  for (int64_t step = 0; step <= m; ++step) {
    const int p = MS_LOAD(parent + v);
    if (p == v) return v;
    if (p < 0 || p > v) break;                                     // not a value of this launch: report, never use it as an address
    const int g = MS_LOAD(parent + p);
    if (g < 0 || g > p) break;
    if (g != p) __hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving: g is an ancestor of v
    v = g;
  }
  *status = 1;
  return -1;
}

// A CAS on parent[hi] fails only if hi has been linked since find_root saw it as a root; hi is then never a root again, so this lane
// never tries hi again, and it can fail on at most m different vertices: the cap of m + 1 cannot be reached.
__device__ __forceinline__ void unite(int32_t* parent, int a, int b, int m, int32_t* status) {
  for (int64_t tries = 0; tries <= m; ++tries) {
    a = find_root(parent, a, m, status);
    b = find_root(parent, b, m, status);
    if (a < 0 || b < 0 || a == b) return;
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  }
  *status = 1;
}

__global__ void __launch_bounds__(MS_THREADS) hook_kernel(const int32_t* __restrict__ faces, int64_t k, int m, int32_t* parent, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (t >= k) return;
  int a, b, c;
  if (!load_face(faces, t, m, a, b, c)) return;
  unite(parent, a, b, m, status);
  unite(parent, b, c, m, status);
}

// In place, plain accesses: what a lane reads is parent[] as the hook launch left it or a root another lane of this launch wrote over
// it, an ancestor either way. The walk descends strictly, so it has fewer than m steps.
__global__ void __launch_bounds__(MS_THREADS) flatten_kernel(int32_t* labels, int m, int32_t* status) {
  const int64_t v0 = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (v0 >= m) return;
  int v = (int)v0;
  for (int64_t step = 0; step <= m; ++step) {
    const int p = labels[v];
    if (p == v) {
      labels[v0] = v;
      return;
    }
    if (p < 0 || p > v) break;
    v = p;
  }
  *status = 1;
}

// out[label] += 1 for every lane with `on`; label must be in range where `on`. Where the wavefront's lanes that are on share one
// label, one of them adds their number once.
__device__ __forceinline__ void add_by_label(int32_t* out, int label, bool on) {
  if (on) {
    const int first = __builtin_amdgcn_readfirstlane(label);
    const unsigned long long active = __ballot(1);
    const unsigned long long same = __ballot(label == first);
    if (same == active) {
      if ((int)(threadIdx.x & 63) == __ffsll((long long)active) - 1) atomicAdd(out + first, (int)__popcll(active));
    } else {
      atomicAdd(out + label, 1);
    }
  }
}

__global__ void __launch_bounds__(MS_THREADS) count_faces_kernel(const int32_t* __restrict__ faces, int64_t k, const int32_t* __restrict__ labels, int m,
                                                                 int32_t* faces_of) {
  const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  int a = 0, b, c, label = 0;
  bool on = t < k && load_face(faces, t, m, a, b, c);
  if (on) {
    label = labels[a];
    on = label >= 0 && label < m;
  }
  add_by_label(faces_of, label, on);
}

// after count_faces_kernel: a vertex counts where its component exists, that is, has a valid face
__global__ void __launch_bounds__(MS_THREADS) count_vertices_kernel(const int32_t* __restrict__ labels, int m, const int32_t* __restrict__ faces_of,
                                                                    int32_t* vertices_of) {
  const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  int label = 0;
  bool on = v < m;
  if (on) {
    label = labels[v];
    on = label >= 0 && label < m && faces_of[label] > 0;
  }
  add_by_label(vertices_of, label, on);
}

__global__ void __launch_bounds__(MS_THREADS) select_kernel(const int32_t* __restrict__ faces, int64_t k, const int32_t* __restrict__ labels, int m,
                                                            const uint8_t* __restrict__ keep_component, uint8_t* __restrict__ face_keep,
                                                            uint8_t* vertex_used) {
  const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (t >= k) return;
  int a, b, c;
  bool keep = load_face(faces, t, m, a, b, c);
  if (keep) {
    const int label = labels[a];
    keep = label >= 0 && label < m && keep_component[label] != 0;
  }
  face_keep[t] = keep ? 1 : 0;
  if (keep) {
    vertex_used[a] = 1;
    vertex_used[b] = 1;
    vertex_used[c] = 1;
  }
}

// lane i moves vertex i (i < m) and face i (i < k)
__global__ void __launch_bounds__(MS_THREADS) compact_kernel(const float* __restrict__ vertices, const uint8_t* __restrict__ colours, int m,
                                                             const int32_t* __restrict__ faces, int64_t k, const uint8_t* __restrict__ face_keep,
                                                             const int32_t* __restrict__ face_rank, const uint8_t* __restrict__ vertex_used,
                                                             const int32_t* __restrict__ vertex_rank, float* __restrict__ out_vertices,
                                                             uint8_t* __restrict__ out_colours, int n_vertices, int32_t* __restrict__ out_faces,
                                                             int n_faces) {
  const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (i < m && vertex_used[i]) {
    const int64_t row = (int64_t)vertex_rank[i] - 1;
    if (row >= 0 && row < n_vertices) {
      for (int c = 0; c < 3; ++c) out_vertices[3 * row + c] = vertices[3 * i + c];
      if (colours)
        for (int c = 0; c < 3; ++c) out_colours[3 * row + c] = colours[3 * i + c];
    }
  }
  if (i < k && face_keep[i]) {
    const int64_t row = (int64_t)face_rank[i] - 1;
    if (row >= 0 && row < n_faces) {
      for (int c = 0; c < 3; ++c) {
        const int v = faces[3 * i + c];
        const int renamed = v >= 0 && v < m ? vertex_rank[v] - 1 : -1;
        out_faces[3 * row + c] = renamed >= 0 && renamed < n_vertices ? renamed : -1;
      }
    }
  }
}

}  // namespace

extern "C" int acez_mesh_components(const int32_t* d_faces, int64_t k, int64_t m, int32_t* d_labels, int32_t* d_status, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE(d_status && (m == 0 || d_labels) && (k == 0 || d_faces), "null pointer");
  if (int rc = acez::require_device("mesh components are labelled on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
  if (m == 0) return ACEZ_OK;
  hipLaunchKernelGGL(init_kernel, dim3(blocks_for(m, MS_THREADS)), dim3(MS_THREADS), 0, s, d_labels, (int)m);
  if (k > 0) hipLaunchKernelGGL(hook_kernel, dim3(blocks_for(k, MS_THREADS)), dim3(MS_THREADS), 0, s, d_faces, k, (int)m, d_labels, d_status);
  hipLaunchKernelGGL(flatten_kernel, dim3(blocks_for(m, MS_THREADS)), dim3(MS_THREADS), 0, s, d_labels, (int)m, d_status);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mesh_component_counts(const int32_t* d_faces, int64_t k, const int32_t* d_labels, int64_t m, int32_t* d_faces_of,
                                          int32_t* d_vertices_of, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE((m == 0 || (d_labels && d_faces_of && d_vertices_of)) && (k == 0 || d_faces), "null pointer");
  if (int rc = acez::require_device("mesh components are counted on a gfx950 GPU")) return rc;
  if (m == 0) return ACEZ_OK;
  hipStream_t s = (hipStream_t)stream;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_faces_of, 0, sizeof(int32_t) * (size_t)m, s));
  ACEZ_HIP_CHECK(hipMemsetAsync(d_vertices_of, 0, sizeof(int32_t) * (size_t)m, s));
  if (k == 0) return ACEZ_OK;
  hipLaunchKernelGGL(count_faces_kernel, dim3(blocks_for(k, MS_THREADS)), dim3(MS_THREADS), 0, s, d_faces, k, d_labels, (int)m, d_faces_of);
  hipLaunchKernelGGL(count_vertices_kernel, dim3(blocks_for(m, MS_THREADS)), dim3(MS_THREADS), 0, s, d_labels, (int)m, (const int32_t*)d_faces_of,
                     d_vertices_of);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mesh_select(const int32_t* d_faces, int64_t k, const int32_t* d_labels, int64_t m, const uint8_t* d_keep_component,
                                uint8_t* d_face_keep, uint8_t* d_vertex_used, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE((m == 0 || (d_labels && d_keep_component && d_vertex_used)) && (k == 0 || (d_faces && d_face_keep)), "null pointer");
  if (int rc = acez::require_device("mesh components are selected on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (m > 0) ACEZ_HIP_CHECK(hipMemsetAsync(d_vertex_used, 0, (size_t)m, s));
  if (k == 0) return ACEZ_OK;
  hipLaunchKernelGGL(select_kernel, dim3(blocks_for(k, MS_THREADS)), dim3(MS_THREADS), 0, s, d_faces, k, d_labels, (int)m, d_keep_component, d_face_keep,
                     d_vertex_used);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_mesh_compact(const float* d_vertices, const uint8_t* d_colours, int64_t m, const int32_t* d_faces, int64_t k,
                                 const uint8_t* d_face_keep, const int32_t* d_face_rank, const uint8_t* d_vertex_used,
                                 const int32_t* d_vertex_rank, float* d_out_vertices, uint8_t* d_out_colours, int64_t n_vertices,
                                 int32_t* d_out_faces, int64_t n_faces, void* stream) {
  ACEZ_REQUIRE_COUNTS(m, k);
  ACEZ_REQUIRE(n_vertices >= 0 && n_vertices <= m && n_faces >= 0 && n_faces <= k, "more output rows than input rows, or a negative number");
  ACEZ_REQUIRE((d_colours == nullptr) == (d_out_colours == nullptr), "vertex colours and output colours go together");
  ACEZ_REQUIRE((m == 0 || (d_vertices && d_vertex_used && d_vertex_rank)) && (k == 0 || (d_faces && d_face_keep && d_face_rank)), "null pointer");
  ACEZ_REQUIRE((n_vertices == 0 || d_out_vertices) && (n_faces == 0 || d_out_faces), "null pointer");
  if (int rc = acez::require_device("meshes are compacted on a gfx950 GPU")) return rc;
  const int64_t lanes = m > k ? m : k;
  if (lanes == 0) return ACEZ_OK;
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(lanes, MS_THREADS)), dim3(MS_THREADS), 0, (hipStream_t)stream, d_vertices, d_colours, (int)m, d_faces, k,
                     d_face_keep, d_face_rank, d_vertex_used, d_vertex_rank, d_out_vertices, d_out_colours, (int)n_vertices, d_out_faces, (int)n_faces);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
