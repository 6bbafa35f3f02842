// meshrender_api.hip -- triangle meshes rendered into the frames' cameras: model depth, face ids, normals and colours per pixel
// (include/acez.h section R, acez_meshrender, acez_meshrender_check_faces).
//
// One call renders every frame of the table in three steps on the caller's stream:
//   1. clear       the call's 64-bit keys to ~0 and the status word to 0 (two memsets);
//   2. raster      one lane per face; a block walks the frames of its grid row with the face's world vertices in registers. Per
//                  frame the lane transforms, culls, clips and sets its triangle up, and the snapped bounding box picks the route:
//                    small   (unclipped, at most ACEZ_MESHRENDER_SMALL samples)   the lane walks its own box;
//                    medium  (up to ACEZ_MESHRENDER_LARGE samples, or clipped)    the wavefront takes the flagged lanes one by one
//                            (a ballot), reads the owner's camera-space vertices by lane shuffles and walks the box with 64 lanes;
//                    large   (more samples)                                       the owners queue their vertices in LDS and the
//                            workgroup walks each queued box with its 256 threads.
//                  Every route runs the same set-up and the same per-sample code, so which route a triangle takes cannot change a
//                  key; a sample is a 64-bit atomicMin of (depth bits << 32 | face id);
//   3. resolve     one thread per pixel: the requested planes from the winning key.
// Positive float depths order like their bit patterns, so the nearest face wins and, at equal depth, the lower id: the image does not
// depend on the order in which the atomics land. The rules are section H's (render_api.hip) in section K's camera: near-plane
// clipping in camera space, 1/256 px snapping, int64 edge functions with the top-left rule. Every float operation is written out in
// the order tests/meshrender_restated.py restates it; the unit is built with -ffp-contract=off.
#include <math.h>
#include <stdint.h>
#include "acez_common.h"
#include "frame_table.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int64_t MR_SUB = 256;                 // sub-pixel steps of the snapped vertices
constexpr float MR_GUARD = 2097152.0f;          // a projected vertex 2^21 px or more off the principal point drops the triangle
constexpr float MR_MAX_PP = 1048576.0f;         // |ppx|, |ppy| <= 2^20: snapped coordinates stay below 1.5 * 2^29 and the int64 edge
                                                // functions below 2^63
constexpr int MR_SMALL = ACEZ_MESHRENDER_SMALL;
constexpr int MR_LARGE = ACEZ_MESHRENDER_LARGE;
constexpr unsigned long long MR_EMPTY = ~0ull;

struct P3 { float x, y, z; };                   // a camera-space point (OpenCV camera: z forward)

__device__ __forceinline__ P3 to_camera(const acez_tsdf_frame& fr, float px, float py, float pz) {
  P3 c;
  c.x = ((fr.m[0] * px + fr.m[1] * py) + fr.m[2] * pz) + fr.m[3];
  c.y = ((fr.m[4] * px + fr.m[5] * py) + fr.m[6] * pz) + fr.m[7];
  c.z = ((fr.m[8] * px + fr.m[9] * py) + fr.m[10] * pz) + fr.m[11];
  return c;
}

__device__ __forceinline__ P3 clip_point(const P3& a, const P3& b, float znear) {   // a inside, b outside
  const float t = (znear - a.z) / (b.z - a.z);
  return P3{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), znear};
}

__device__ __forceinline__ int64_t edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// top-left rule (render_api.hip): of two triangles that share an edge exactly one owns a sample on it
__device__ __forceinline__ bool owns_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (by - ay) > 0 || ((by - ay) == 0 && (bx - ax) < 0);
}

// a projected triangle ready to be walked
struct Setup {
  int64_t X[3], Y[3], area;
  float iz[3];
  int x0, y0, bw, count;                        // the box's first pixel, its width and its samples; count == 0: nothing to draw
  bool guard;                                   // dropped by the 2^21 guard
};

__device__ Setup setup_triangle(const acez_tsdf_frame& fr, const P3& p0, const P3& p1, const P3& p2) {
  Setup s;
  s.count = 0;
  s.guard = false;
  const P3* p[3] = {&p0, &p1, &p2};
  float u[3], v[3];
  for (int k = 0; k < 3; ++k) {
    const float a = (fr.focal * p[k]->x) / p[k]->z, b = (fr.focal * p[k]->y) / p[k]->z;
    if (!(fabsf(a) < MR_GUARD && fabsf(b) < MR_GUARD)) s.guard = true;
    u[k] = a + fr.ppx;
    v[k] = b + fr.ppy;
    s.iz[k] = 1.0f / p[k]->z;
  }
  if (s.guard) return s;
  for (int k = 0; k < 3; ++k) {
    s.X[k] = (int64_t)rintf(u[k] * (float)MR_SUB);
    s.Y[k] = (int64_t)rintf(v[k] * (float)MR_SUB);
  }
  s.area = edge(s.X[0], s.Y[0], s.X[1], s.Y[1], s.X[2], s.Y[2]);
  if (s.area == 0) return s;
  if (s.area < 0) {                             // both windings are drawn: make it positive by swapping vertices 1 and 2
    int64_t t = s.X[1]; s.X[1] = s.X[2]; s.X[2] = t;
    t = s.Y[1]; s.Y[1] = s.Y[2]; s.Y[2] = t;
    const float f = s.iz[1]; s.iz[1] = s.iz[2]; s.iz[2] = f;
    s.area = -s.area;
  }
  const int64_t xmin = min(s.X[0], min(s.X[1], s.X[2])), xmax = max(s.X[0], max(s.X[1], s.X[2]));
  const int64_t ymin = min(s.Y[0], min(s.Y[1], s.Y[2])), ymax = max(s.Y[0], max(s.Y[1], s.Y[2]));
  // the pixels whose sample point (ix, iy) lies in the box: ceil(min / 256) .. floor(max / 256), cut to the image
  const int64_t x0 = max((int64_t)0, (xmin + MR_SUB - 1) >> 8), x1 = min((int64_t)fr.w - 1, xmax >> 8);
  const int64_t y0 = max((int64_t)0, (ymin + MR_SUB - 1) >> 8), y1 = min((int64_t)fr.h - 1, ymax >> 8);
  if (x1 < x0 || y1 < y0) return s;
  s.x0 = (int)x0;
  s.y0 = (int)y0;
  s.bw = (int)(x1 - x0 + 1);
  s.count = s.bw * (int)(y1 - y0 + 1);          // at most 32768^2 = 2^30
  return s;
}

// samples start, start + stride, .. of the box. Every pixel index lies inside the frame (set-up cut the box to it), and the frame
// inside the key buffer (the host checked the row).
__device__ void walk(const Setup& s, const acez_tsdf_frame& fr, float max_depth, uint32_t id, unsigned long long* __restrict__ keys,
                     int start, int stride) {
  if (s.count == 0) return;
  const bool t0 = owns_edge(s.X[1], s.Y[1], s.X[2], s.Y[2]), t1 = owns_edge(s.X[2], s.Y[2], s.X[0], s.Y[0]),
             t2 = owns_edge(s.X[0], s.Y[0], s.X[1], s.Y[1]);
  const float farea = (float)s.area;
  for (int j = start; j < s.count; j += stride) {
    const int px = s.x0 + j % s.bw, py = s.y0 + j / s.bw;
    const int64_t sx = (int64_t)px * MR_SUB, sy = (int64_t)py * MR_SUB;
    const int64_t w0 = edge(s.X[1], s.Y[1], s.X[2], s.Y[2], sx, sy);
    const int64_t w1 = edge(s.X[2], s.Y[2], s.X[0], s.Y[0], sx, sy);
    const int64_t w2 = edge(s.X[0], s.Y[0], s.X[1], s.Y[1], sx, sy);
    if (w0 < 0 || w1 < 0 || w2 < 0) continue;
    if ((w0 == 0 && !t0) || (w1 == 0 && !t1) || (w2 == 0 && !t2)) continue;
    const float invd = (((float)w0 * s.iz[0] + (float)w1 * s.iz[1]) + (float)w2 * s.iz[2]) / farea;   // perspective-correct 1 / depth
    const float d = 1.0f / invd;
    if (!(d <= max_depth)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)id;
    atomicMin(keys + fr.offset + (int64_t)py * fr.w + px, key);
  }
}

// what is left of a camera-space triangle in front of the near plane: 0, 3 or 4 points (Sutherland-Hodgman over the edges (0,1),
// (1,2), (2,0); a quad is drawn as the fan (0,1,2), (0,2,3))
__device__ int clip_near(const P3 v[3], float znear, P3 poly[4]) {
  bool in[3];
  int n_in = 0;
  for (int k = 0; k < 3; ++k) {
    in[k] = v[k].z >= znear;
    n_in += in[k] ? 1 : 0;
  }
  if (n_in == 0) return 0;
  if (n_in == 3) {
    poly[0] = v[0]; poly[1] = v[1]; poly[2] = v[2];
    return 3;
  }
  int np = 0;
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1;
    if (in[k]) poly[np++] = v[k];
    if (in[k] != in[k1]) poly[np++] = in[k] ? clip_point(v[k], v[k1], znear) : clip_point(v[k1], v[k], znear);
  }
  return np;
}

// a whole triangle-frame with `stride` threads: clip, set up, walk. The medium and the large route.
__device__ void draw_shared(const acez_tsdf_frame& fr, const P3 v[3], float min_depth, float max_depth, uint32_t id,
                            unsigned long long* __restrict__ keys, int start, int stride) {
  P3 poly[4];
  const int np = clip_near(v, min_depth, poly);
  if (np >= 3) {
    const Setup s = setup_triangle(fr, poly[0], poly[1], poly[2]);
    walk(s, fr, max_depth, id, keys, start, stride);
  }
  if (np == 4) {
    const Setup s = setup_triangle(fr, poly[0], poly[2], poly[3]);
    walk(s, fr, max_depth, id, keys, start, stride);
  }
}

struct Queued { P3 v[3]; uint32_t id; };

__global__ void __launch_bounds__(MR_THREADS) meshrender_raster_kernel(const float* __restrict__ vertices, int64_t n_vertices,
                                                                       const int32_t* __restrict__ faces, int64_t n_faces,
                                                                       const acez_tsdf_frame* __restrict__ frames, int n_frames,
                                                                       float min_depth, float max_depth,
                                                                       unsigned long long* __restrict__ keys, int32_t* __restrict__ status) {
  __shared__ Queued queue[MR_THREADS];
  __shared__ int queued;
  const int lane = threadIdx.x & 63;
  const int64_t blocks = (n_faces + MR_THREADS - 1) / MR_THREADS;
  for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {        // uniform over the block: the barriers below are safe
    const int64_t t = b * MR_THREADS + threadIdx.x;
    float w[9];
    bool have = false;
    if (t < n_faces) {
      const int32_t i0 = faces[3 * t], i1 = faces[3 * t + 1], i2 = faces[3 * t + 2];
      have = (uint64_t)i0 < (uint64_t)n_vertices && (uint64_t)i1 < (uint64_t)n_vertices && (uint64_t)i2 < (uint64_t)n_vertices;
      if (have) {                                                    // (a negative index is a huge unsigned one)
        const int32_t idx[3] = {i0, i1, i2};
        for (int k = 0; k < 3; ++k)
          for (int c = 0; c < 3; ++c) w[3 * k + c] = vertices[3 * (int64_t)idx[k] + c];
      }
    }
    const uint32_t id = (uint32_t)t;
    for (int f = blockIdx.y; f < n_frames; f += gridDim.y) {
      const acez_tsdf_frame fr = frames[f];
      // ---- the lane's own triangle-frame: transform, cull, classify; a small one is drawn at once
      int route = 0;                                                 // 0 nothing more to do, 1 medium, 2 large
      P3 v[3] = {};
      if (have) {
        bool finite = true;
        for (int k = 0; k < 3; ++k) {
          v[k] = to_camera(fr, w[3 * k], w[3 * k + 1], w[3 * k + 2]);
          finite = finite && isfinite(v[k].x) && isfinite(v[k].y) && isfinite(v[k].z);
        }
        P3 poly[4];
        const int np = finite ? clip_near(v, min_depth, poly) : 0;
        if (np >= 3) {
          const bool clipped = !(v[0].z >= min_depth && v[1].z >= min_depth && v[2].z >= min_depth);
          const Setup s = setup_triangle(fr, poly[0], poly[1], poly[2]);
          bool guard = s.guard;
          int most = s.count;
          if (np == 4) {
            const Setup s2 = setup_triangle(fr, poly[0], poly[2], poly[3]);
            guard = guard || s2.guard;
            most = max(most, s2.count);
          }
          if (guard) atomicAdd(status, 1);
          if (most > MR_LARGE) route = 2;
          else if (most > MR_SMALL || (clipped && most > 0)) route = 1;
          else if (most > 0) walk(s, fr, max_depth, id, keys, 0, 1);
        }
      }
      // ---- medium: the wavefront takes its flagged lanes in turn
      unsigned long long todo = __ballot(route == 1);
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        P3 sv[3];
        for (int k = 0; k < 3; ++k) {
          sv[k].x = __shfl(v[k].x, src);
          sv[k].y = __shfl(v[k].y, src);
          sv[k].z = __shfl(v[k].z, src);
        }
        const uint32_t sid = (uint32_t)__shfl((int)id, src);
        draw_shared(fr, sv, min_depth, max_depth, sid, keys, lane, 64);
      }
      // ---- large: queued in LDS, each walked by the whole workgroup
      if (threadIdx.x == 0) queued = 0;
      __syncthreads();
      if (route == 2) {
        const int at = atomicAdd(&queued, 1);                        // the order in the queue changes no key
        queue[at].v[0] = v[0]; queue[at].v[1] = v[1]; queue[at].v[2] = v[2];
        queue[at].id = id;
      }
      __syncthreads();
      const int n_queued = queued;
      for (int q = 0; q < n_queued; ++q) {
        const P3 qv[3] = {queue[q].v[0], queue[q].v[1], queue[q].v[2]};
        draw_shared(fr, qv, min_depth, max_depth, queue[q].id, keys, threadIdx.x, MR_THREADS);
      }
      __syncthreads();                                               // the queue is free for the next frame
    }
  }
}

__device__ __forceinline__ uint8_t unit_to_byte(float c) {           // 128 + rint(127 c), c in [-1, 1]: 1 .. 255
  const float q = rintf(c * 127.0f) + 128.0f;
  return (uint8_t)(int)fminf(fmaxf(q, 1.0f), 255.0f);
}

__global__ void __launch_bounds__(MR_THREADS) meshrender_resolve_kernel(const float* __restrict__ vertices, const uint8_t* __restrict__ colours,
                                                                        const int32_t* __restrict__ faces,
                                                                        const acez_tsdf_frame* __restrict__ frames, float depth_unit,
                                                                        const unsigned long long* __restrict__ keys, float* __restrict__ out_depth,
                                                                        int32_t* __restrict__ out_face, uint16_t* __restrict__ out_u16,
                                                                        uint8_t* __restrict__ out_normal, uint8_t* __restrict__ out_colour) {
  const acez_tsdf_frame fr = frames[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * MR_THREADS + threadIdx.x;
  if (i >= (int64_t)fr.h * fr.w) return;
  const int64_t o = fr.offset + i;
  const unsigned long long key = keys[o];
  const bool hit = key != MR_EMPTY;
  const float d = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
  const int32_t id = hit ? (int32_t)(uint32_t)(key & 0xffffffffull) : -1;
  if (out_depth) out_depth[o] = d;
  if (out_face) out_face[o] = id;
  if (out_u16) {
    const float q = rintf(d / depth_unit);
    out_u16[o] = hit && q <= 65535.0f ? (uint16_t)q : (uint16_t)0;
  }
  if (!out_normal && !out_colour) return;
  uint8_t nrm[3] = {0, 0, 0}, rgb[3] = {0, 0, 0};
  if (hit) {
    // only a face whose three indices are in range writes a key
    const int32_t idx[3] = {faces[3 * (int64_t)id], faces[3 * (int64_t)id + 1], faces[3 * (int64_t)id + 2]};
    P3 p[3];
    for (int k = 0; k < 3; ++k)
      p[k] = to_camera(fr, vertices[3 * (int64_t)idx[k]], vertices[3 * (int64_t)idx[k] + 1], vertices[3 * (int64_t)idx[k] + 2]);
    const int ix = (int)(i % fr.w), iy = (int)(i / fr.w);
    const float rx = (float)ix - fr.ppx, ry = (float)iy - fr.ppy, rz = fr.focal;     // the pixel's ray, up to the factor 1 / focal
    if (out_normal) {
      const float ax = p[1].x - p[0].x, ay = p[1].y - p[0].y, az = p[1].z - p[0].z;
      const float bx = p[2].x - p[0].x, by = p[2].y - p[0].y, bz = p[2].z - p[0].z;
      float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
      const float along = (nx * rx + ny * ry) + nz * rz;
      if (along > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }             // towards the camera
      const float len = (float)sqrt((double)((nx * nx + ny * ny) + nz * nz));
      if (len > 0.0f && len < INFINITY) {
        nrm[0] = unit_to_byte(nx / len); nrm[1] = unit_to_byte(ny / len); nrm[2] = unit_to_byte(nz / len);
      } else {
        nrm[0] = nrm[1] = nrm[2] = 128;                               // no direction (the squares under- or overflowed)
      }
    }
    if (out_colour) {
      // C_k = P_(k+1) x P_(k+2); e_k = ray . C_k are the barycentrics up to their sum (render_api.hip's textured path): they come
      // from the unclipped vertices, so near-plane clipping does not change them
      float e[3];
      for (int k = 0; k < 3; ++k) {
        const P3& a = p[k == 2 ? 0 : k + 1];
        const P3& b = p[k == 0 ? 2 : k - 1];
        const float cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
        e[k] = (rx * cx + ry * cy) + rz * cz;
      }
      const float D = (e[0] + e[1]) + e[2];
      for (int c = 0; c < 3; ++c) {
        const float m = ((e[0] * (float)colours[3 * (int64_t)idx[0] + c] + e[1] * (float)colours[3 * (int64_t)idx[1] + c]) +
                         e[2] * (float)colours[3 * (int64_t)idx[2] + c]) / D;
        const float q = floorf(m + 0.5f);
        rgb[c] = q >= 0.0f ? (uint8_t)(int)fminf(q, 255.0f) : (uint8_t)0;      // (a NaN gives 0)
      }
    }
  }
  if (out_normal) { out_normal[3 * o] = nrm[0]; out_normal[3 * o + 1] = nrm[1]; out_normal[3 * o + 2] = nrm[2]; }
  if (out_colour) { out_colour[3 * o] = rgb[0]; out_colour[3 * o + 1] = rgb[1]; out_colour[3 * o + 2] = rgb[2]; }
}

}  // namespace

extern "C" int acez_meshrender_check_faces(const int32_t* h_faces, int64_t n_faces, int64_t n_vertices) {
  ACEZ_REQUIRE(n_faces >= 0 && n_faces < ((int64_t)1 << 31), "face count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31), "vertex count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(n_faces == 0 || h_faces, "null pointer");
  for (int64_t i = 0; i < 3 * n_faces; ++i)
    ACEZ_REQUIRE(h_faces[i] >= 0 && h_faces[i] < n_vertices, "face index outside the vertices");
  return ACEZ_OK;
}

extern "C" int acez_meshrender(const float* d_vertices, const uint8_t* d_colours, int64_t n_vertices, const int32_t* d_faces,
                               int64_t n_faces, const acez_tsdf_frame* h_frames, int n_frames, acez_tsdf_frame* d_frames, float min_depth,
                               float max_depth, float depth_unit, unsigned long long* d_keys, int64_t n_keys, float* d_depth,
                               int32_t* d_face, uint16_t* d_depth_u16, uint8_t* d_normal, uint8_t* d_colour, int64_t n_pixels,
                               int32_t* d_status, void* stream) {
  ACEZ_REQUIRE(n_faces >= 0 && n_faces < ((int64_t)1 << 31), "face count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31), "vertex count out of range (0 .. 2^31 - 1)");
  ACEZ_REQUIRE(n_faces == 0 || (d_faces && d_vertices && n_vertices > 0), "faces without indices or vertices");
  ACEZ_REQUIRE(d_keys && d_depth && d_status, "null pointer (keys, depth or status)");
  ACEZ_REQUIRE(!d_colour || d_colours || n_faces == 0, "a colour plane needs vertex colours");
  ACEZ_REQUIRE(min_depth > 0.0f && isfinite(min_depth), "min_depth must be positive and finite");
  ACEZ_REQUIRE(max_depth > 0.0f && isfinite(max_depth), "max_depth must be positive and finite");
  ACEZ_REQUIRE(depth_unit > 0.0f && isfinite(depth_unit), "depth_unit must be positive and finite");
  ACEZ_REQUIRE(n_frames >= 0 && n_frames <= ACEZ_TSDF_MAX_FRAMES, "frame count out of range (0 .. 256)");
  ACEZ_REQUIRE(n_keys >= 0 && n_pixels >= 0, "negative buffer length");
  if (n_frames == 0) return ACEZ_OK;
  ACEZ_REQUIRE(h_frames && d_frames, "null frame table");
  int64_t extent = 0, largest = 0;
  for (int f = 0; f < n_frames; ++f) {
    if (int rc = acez::check_frame(h_frames[f], n_pixels < n_keys ? n_pixels : n_keys)) return rc;
    ACEZ_REQUIRE(fabsf(h_frames[f].ppx) <= MR_MAX_PP && fabsf(h_frames[f].ppy) <= MR_MAX_PP, "principal point more than 2^20 px from the origin");
    const int64_t px = (int64_t)h_frames[f].h * h_frames[f].w;
    extent = extent > h_frames[f].offset + px ? extent : h_frames[f].offset + px;
    largest = largest > px ? largest : px;
  }
  if (int rc = acez::require_device("mesh rendering runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = acez::upload_frames(d_frames, h_frames, n_frames, s)) return rc;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_keys, 0xff, (size_t)extent * sizeof(unsigned long long), s));
  ACEZ_HIP_CHECK(hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
  if (n_faces > 0) {
    // a block keeps its faces in registers over the frames of its grid row: few face blocks spread the frames over the grid's rows
    const int64_t blocks = (n_faces + MR_THREADS - 1) / MR_THREADS;
    const int gx = (int)(blocks < 1048576 ? blocks : 1048576);
    int64_t gy = (4096 + blocks - 1) / blocks;
    gy = gy < 1 ? 1 : (gy > n_frames ? n_frames : gy);
    hipLaunchKernelGGL(meshrender_raster_kernel, dim3(gx, (int)gy), dim3(MR_THREADS), 0, s, d_vertices, n_vertices, d_faces, n_faces,
                       (const acez_tsdf_frame*)d_frames, n_frames, min_depth, max_depth, d_keys, d_status);
    ACEZ_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(meshrender_resolve_kernel, dim3((unsigned)((largest + MR_THREADS - 1) / MR_THREADS), n_frames), dim3(MR_THREADS), 0, s,
                     d_vertices, d_colours, d_faces, (const acez_tsdf_frame*)d_frames, depth_unit, (const unsigned long long*)d_keys, d_depth,
                     d_face, d_depth_u16, d_normal, d_colour);
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}
