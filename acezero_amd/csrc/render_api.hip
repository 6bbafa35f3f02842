// render_api.hip -- headless rasteriser of the reconstruction video (include/acez.h section H, acez_render_frame,
// acez_render_frame_tex, acez_render_texture_build).
//
// One frame is four steps on the caller's stream:
//   1. clear       both 64-bit key planes to ~0 (one memset);
//   2. points      one thread per point: transform, project, and a 64-bit atomicMin of (depth bits << 32 | point index) into each
//                  pixel of its 2 x 2 px square (the reference's point_size = 2);
//   3. triangles   one wavefront per triangle: clip against the near plane in camera space (0, 1 or 2 triangles remain), snap the
//                  projected vertices to 1/256 px, and let the 64 lanes walk the bounding box; a pixel is covered when the exact
//                  integer edge functions at its centre pass the top-left rule; atomicMin of (depth bits << 32 | triangle id);
//                  Textured triangles (acez_render_frame_tex: the image thumbnails in the registration frustums) go through the
//                  same code with ids after the flat ones, into the same key plane;
//   4. resolve     one thread per output pixel: the winning point's colour (black if none), the winning triangle's RGBA blended on
//                  top in double precision and truncated (the reference's _blend_images), rotated -90 degrees for a flipped
//                  portrait frame. A pixel won by a textured triangle takes its trilinearly filtered texel (shade_textured).
// Positive float depths order like their bit patterns, so the packed key makes the nearest primitive win and, at equal depth, the
// lower index: the result does not depend on the order in which the atomics land. The layers do not depth-test against each other.
// Every float operation is written out in the order tests/render_oracle.py and tests/render_texture_oracle.py restate it; the unit is
// built with -ffp-contract=off, and the textured path uses only + - * /, comparisons, floor and the exponent / mantissa bits of a float.
#include <math.h>
#include <stdint.h>
#include "acez_common.h"

namespace {

constexpr int RT_THREADS = 256;
constexpr int64_t RT_SUB = 256;                 // sub-pixel steps of the snapped triangle vertices
constexpr float RT_GUARD = 2097152.0f;          // |projected coordinate| of 2^21 px or more: the triangle is dropped (keeps the
                                                // int64 edge functions of 1/256 px coordinates far from overflow)

struct Cam {
  float m[12];                                  // world -> camera rows (OpenGL camera: looks down -z)
  float f, cx, cy, znear, zfar;
  int W, H;
};

__device__ __forceinline__ void to_camera(const Cam& c, float x, float y, float z, float& xc, float& yc, float& zc) {
  xc = c.m[0] * x + c.m[1] * y + c.m[2] * z + c.m[3];
  yc = c.m[4] * x + c.m[5] * y + c.m[6] * z + c.m[7];
  zc = c.m[8] * x + c.m[9] * y + c.m[10] * z + c.m[11];
}

__global__ void __launch_bounds__(RT_THREADS) splat_points_kernel(const float* __restrict__ xyz, int64_t n, Cam c,
                                                                  unsigned long long* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RT_THREADS) {
    float xc, yc, zc;
    to_camera(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xc, yc, zc);
    const float d = -zc;
    if (!(d >= c.znear && d <= c.zfar)) continue;          // behind the camera, outside the planes, or NaN
    const float u = c.cx + (c.f * xc) / d;
    const float v = c.cy - (c.f * yc) / d;
    if (!(u > -2.0f && u < (float)c.W + 2.0f && v > -2.0f && v < (float)c.H + 2.0f)) continue;
    const int x0 = (int)floorf(u - 0.5f), y0 = (int)floorf(v - 0.5f);   // the 2 x 2 pixels whose centres are nearest to (u, v)
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(uint32_t)i;
    for (int dy = 0; dy < 2; ++dy) {
      const int y = y0 + dy;
      if (y < 0 || y >= c.H) continue;
      for (int dx = 0; dx < 2; ++dx) {
        const int x = x0 + dx;
        if (x < 0 || x >= c.W) continue;
        atomicMin(keys + (int64_t)y * c.W + x, key);
      }
    }
  }
}

struct Vtx { float x, y, d; };                 // camera-space x, y and depth d = -z

__device__ __forceinline__ Vtx clip_point(const Vtx& a, const Vtx& b, float znear) {   // a inside, b outside
  const float t = (znear - a.d) / (b.d - a.d);
  return Vtx{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), znear};
}

__device__ __forceinline__ int64_t edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

// top-left rule: a sample exactly on an edge belongs to the triangle only for the edges that satisfy this (for the same edge walked
// the other way round the test is false, so two triangles sharing an edge never both take or both miss a sample on it)
__device__ __forceinline__ bool owns_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return (by - ay) > 0 || ((by - ay) == 0 && (bx - ax) < 0);
}

// rasterise one projected (and possibly clipped) triangle with the 64 lanes of a wavefront
__device__ void raster_wave(const Cam& c, const Vtx& p0, const Vtx& p1, const Vtx& p2, uint32_t id, unsigned long long* keys, int lane) {
  float u[3], v[3], iz[3];
  const Vtx* p[3] = {&p0, &p1, &p2};
  for (int k = 0; k < 3; ++k) {
    u[k] = c.cx + (c.f * p[k]->x) / p[k]->d;
    v[k] = c.cy - (c.f * p[k]->y) / p[k]->d;
    iz[k] = 1.0f / p[k]->d;
    if (!(fabsf(u[k]) < RT_GUARD && fabsf(v[k]) < RT_GUARD)) return;
  }
  int64_t X[3], Y[3];
  for (int k = 0; k < 3; ++k) {
    X[k] = (int64_t)rintf(u[k] * (float)RT_SUB);
    Y[k] = (int64_t)rintf(v[k] * (float)RT_SUB);
  }
  int64_t area = edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
  if (area == 0) return;
  if (area < 0) {                                // both windings are drawn: make it positive by swapping vertices 1 and 2
    int64_t t = X[1]; X[1] = X[2]; X[2] = t;
    t = Y[1]; Y[1] = Y[2]; Y[2] = t;
    float f = iz[1]; iz[1] = iz[2]; iz[2] = f;
    area = -area;
  }
  int64_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
  int64_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
  // pixels whose centre (px + 1/2) lies in the box
  int x0 = (int)max((int64_t)0, (xmin - RT_SUB / 2 + RT_SUB - 1) >> 8);
  int x1 = (int)min((int64_t)c.W - 1, (xmax - RT_SUB / 2) >> 8);
  int y0 = (int)max((int64_t)0, (ymin - RT_SUB / 2 + RT_SUB - 1) >> 8);
  int y1 = (int)min((int64_t)c.H - 1, (ymax - RT_SUB / 2) >> 8);
  if (x1 < x0 || y1 < y0) return;
  const bool t0 = owns_edge(X[1], Y[1], X[2], Y[2]), t1 = owns_edge(X[2], Y[2], X[0], Y[0]), t2 = owns_edge(X[0], Y[0], X[1], Y[1]);
  const float farea = (float)area;
  const int bw = x1 - x0 + 1;
  const int64_t count = (int64_t)bw * (y1 - y0 + 1);
  for (int64_t j = lane; j < count; j += 64) {
    const int px = x0 + (int)(j % bw), py = y0 + (int)(j / bw);
    const int64_t sx = (int64_t)px * RT_SUB + RT_SUB / 2, sy = (int64_t)py * RT_SUB + RT_SUB / 2;
    const int64_t w0 = edge(X[1], Y[1], X[2], Y[2], sx, sy);
    const int64_t w1 = edge(X[2], Y[2], X[0], Y[0], sx, sy);
    const int64_t w2 = edge(X[0], Y[0], X[1], Y[1], sx, sy);
    if (w0 < 0 || w1 < 0 || w2 < 0) continue;
    if ((w0 == 0 && !t0) || (w1 == 0 && !t1) || (w2 == 0 && !t2)) continue;
    const float invd = ((float)w0 * iz[0] + (float)w1 * iz[1] + (float)w2 * iz[2]) / farea;   // perspective-correct 1/depth
    const float d = 1.0f / invd;
    if (!(d <= c.zfar)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)id;
    atomicMin(keys + (int64_t)py * c.W + px, key);
  }
}

// one world-space triangle (9 floats) with the 64 lanes of a wavefront: transform, clip against the near plane, rasterise
__device__ void draw_triangle(const Cam& c, const float* xyz, uint32_t id, unsigned long long* keys, int lane) {
  Vtx v[3];
  bool in[3];
  int n_in = 0;
  for (int k = 0; k < 3; ++k) {
    float xc, yc, zc;
    to_camera(c, xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2], xc, yc, zc);
    v[k] = Vtx{xc, yc, -zc};
    if (!(isfinite(xc) && isfinite(yc) && isfinite(zc))) return;
    in[k] = v[k].d >= c.znear;
    n_in += in[k] ? 1 : 0;
  }
  if (n_in == 0) return;                         // wholly in front of the near plane
  if (n_in == 3) {
    raster_wave(c, v[0], v[1], v[2], id, keys, lane);
    return;
  }
  // Sutherland-Hodgman against d >= znear over the edges (0,1), (1,2), (2,0); the result is a triangle or a quad, drawn as a fan
  Vtx poly[4];
  int np = 0;
  for (int k = 0; k < 3; ++k) {
    const int k1 = k == 2 ? 0 : k + 1;
    if (in[k]) poly[np++] = v[k];
    if (in[k] != in[k1]) poly[np++] = in[k] ? clip_point(v[k], v[k1], c.znear) : clip_point(v[k1], v[k], c.znear);
  }
  raster_wave(c, poly[0], poly[1], poly[2], id, keys, lane);
  if (np == 4) raster_wave(c, poly[0], poly[2], poly[3], id, keys, lane);
}

__global__ void __launch_bounds__(RT_THREADS) raster_triangles_kernel(const float* __restrict__ tri, int64_t m, Cam c,
                                                                      unsigned long long* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (RT_THREADS / 64);
  for (int64_t t = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6); t < m; t += waves)
    draw_triangle(c, tri + 9 * t, (uint32_t)t, keys, lane);
}

// ---------------------------------------------------------------------------------------------------------- textured triangles
// The textured triangles and their texture table travel as launch arguments (a few thumbnails per frame): no upload, and every
// index was checked on the host before the launch.
struct TexArgs {
  acez_tex_triangle tri[ACEZ_RENDER_MAX_TEX_TRIANGLES];
  acez_texture tex[ACEZ_RENDER_MAX_TEXTURES];
  const uint8_t* texels;
  int n;                                         // textured triangles
  uint32_t id0;                                  // triangle id of textured triangle 0 (= the number of flat triangles)
  static constexpr bool enabled = true;
};

static_assert(sizeof(acez_tex_triangle) == 68 && sizeof(acez_texture) == 16, "acezero_amd/_native.py mirrors these layouts");

struct NoTex {                                   // acez_render_frame: the resolve without the textured branch
  static constexpr bool enabled = false;
};

__global__ void __launch_bounds__(RT_THREADS) raster_textured_kernel(const TexArgs tx, Cam c, unsigned long long* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
  if (t >= tx.n) return;
  float xyz[9];
  for (int k = 0; k < 9; ++k) xyz[k] = tx.tri[t].xyz[k / 3][k % 3];
  draw_triangle(c, xyz, tx.id0 + (uint32_t)t, keys, lane);
}

// level k of a texture: its first texel and its size (levels follow each other, each max(1, half) of the one before)
__device__ __forceinline__ const uint8_t* tex_level(const uint8_t* texels, const acez_texture& t, int k, int& w, int& h) {
  int64_t off = t.offset;
  w = t.width;
  h = t.height;
  for (int j = 0; j < k; ++j) {
    off += (int64_t)w * h * 3;
    w = max(1, w >> 1);
    h = max(1, h >> 1);
  }
  return texels + off;
}

// bilinear about texel centres, clamp to edge: float RGB in [0, 255]
__device__ void bilinear(const uint8_t* p, int w, int h, float u, float v, float out[3]) {
  float s = u * (float)w - 0.5f, t = v * (float)h - 0.5f;
  if (!(s >= -1.0f)) s = -1.0f;                  // (a NaN coordinate lands here too)
  if (s > (float)w) s = (float)w;
  if (!(t >= -1.0f)) t = -1.0f;
  if (t > (float)h) t = (float)h;
  const float fs = floorf(s), ft = floorf(t);
  const float a = s - fs, b = t - ft;
  const int i0 = min(max((int)fs, 0), w - 1), i1 = min(max((int)fs + 1, 0), w - 1);
  const int j0 = min(max((int)ft, 0), h - 1), j1 = min(max((int)ft + 1, 0), h - 1);
  const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
  const uint8_t* t00 = p + 3 * ((int64_t)j0 * w + i0);
  const uint8_t* t10 = p + 3 * ((int64_t)j0 * w + i1);
  const uint8_t* t01 = p + 3 * ((int64_t)j1 * w + i0);
  const uint8_t* t11 = p + 3 * ((int64_t)j1 * w + i1);
  for (int k = 0; k < 3; ++k) out[k] = ((w00 * (float)t00[k] + w10 * (float)t10[k]) + w01 * (float)t01[k]) + w11 * (float)t11[k];
}

// the texel colour of textured triangle t at render pixel (px, py): perspective-correct uv, trilinear filtering
__device__ void shade_textured(const TexArgs& tx, const Cam& c, int t, int px, int py, uint8_t r[3]) {
  const acez_tex_triangle& T = tx.tri[t];
  float P[3][3];
  for (int k = 0; k < 3; ++k) to_camera(c, T.xyz[k][0], T.xyz[k][1], T.xyz[k][2], P[k][0], P[k][1], P[k][2]);
  // C_k = P_{k+1} x P_{k+2}; the pixel's ray r = (x + 1/2 - cx, cy - y - 1/2, -f) meets the plane at barycentrics e_k / sum(e)
  // with e_k = r . C_k (triple products: exact for any point of the plane, clipped or not)
  float C[3][3];
  for (int k = 0; k < 3; ++k) {
    const float* a = P[k == 2 ? 0 : k + 1];
    const float* b = P[k == 0 ? 2 : k - 1];
    C[k][0] = a[1] * b[2] - a[2] * b[1];
    C[k][1] = a[2] * b[0] - a[0] * b[2];
    C[k][2] = a[0] * b[1] - a[1] * b[0];
  }
  const float rx = ((float)px + 0.5f) - c.cx, ry = c.cy - ((float)py + 0.5f), rz = -c.f;
  float e[3];
  for (int k = 0; k < 3; ++k) e[k] = (rx * C[k][0] + ry * C[k][1]) + rz * C[k][2];
  const float D = (e[0] + e[1]) + e[2];
  const float U = ((e[0] * T.uv[0][0] + e[1] * T.uv[1][0]) + e[2] * T.uv[2][0]) / D;
  const float V = ((e[0] * T.uv[0][1] + e[1] * T.uv[1][1]) + e[2] * T.uv[2][1]) / D;
  // d(e_k)/dx = C_k.x, d(e_k)/dy = -C_k.y: dU/dx = (sum C_k.x u_k - U sum C_k.x) / D (the sign of the y derivatives drops out of rho)
  const float Dx = (C[0][0] + C[1][0]) + C[2][0], Dy = (C[0][1] + C[1][1]) + C[2][1];
  const float Nux = (C[0][0] * T.uv[0][0] + C[1][0] * T.uv[1][0]) + C[2][0] * T.uv[2][0];
  const float Nvx = (C[0][0] * T.uv[0][1] + C[1][0] * T.uv[1][1]) + C[2][0] * T.uv[2][1];
  const float Nuy = (C[0][1] * T.uv[0][0] + C[1][1] * T.uv[1][0]) + C[2][1] * T.uv[2][0];
  const float Nvy = (C[0][1] * T.uv[0][1] + C[1][1] * T.uv[1][1]) + C[2][1] * T.uv[2][1];
  const acez_texture& tex = tx.tex[T.texture];
  const float W0 = (float)tex.width, H0 = (float)tex.height;
  const float sx = ((Nux - U * Dx) / D) * W0, tx_ = ((Nvx - V * Dx) / D) * H0;
  const float sy = ((Nuy - U * Dy) / D) * W0, ty = ((Nvy - V * Dy) / D) * H0;
  const float rho2x = sx * sx + tx_ * tx_, rho2y = sy * sy + ty * ty;
  const float rho2 = rho2y > rho2x ? rho2y : rho2x;
  int q = 0;                                     // last level
  for (int m = max(tex.width, tex.height); m > 1; m >>= 1) ++q;
  int l0 = 0, l1 = -1;
  float frac = 0.0f;
  if (rho2 <= 1.0f) {
    l0 = 0;                                      // lambda <= 0: magnified, level 0
  } else if (!(rho2 < INFINITY)) {
    l0 = q;
  } else {                                       // lambda = (e + (m - 1)) / 2 for rho^2 = m 2^e, m in [1, 2), e >= 0
    const uint32_t bits = __float_as_uint(rho2);
    const int ex = (int)(bits >> 23) - 127;
    const float mf = __uint_as_float((bits & 0x7fffffu) | 0x3f800000u) - 1.0f;
    const int L = ex >> 1;
    frac = ((float)(ex & 1) + mf) * 0.5f;
    if (L >= q) {
      l0 = q;
    } else {
      l0 = L;
      l1 = L + 1;
    }
  }
  int w, h;
  float c0[3];
  bilinear(tex_level(tx.texels, tex, l0, w, h), w, h, U, V, c0);
  if (l1 >= 0) {
    float c1[3];
    bilinear(tex_level(tx.texels, tex, l1, w, h), w, h, U, V, c1);
    for (int k = 0; k < 3; ++k) c0[k] = (1.0f - frac) * c0[k] + frac * c1[k];
  }
  for (int k = 0; k < 3; ++k) {
    const int v = (int)(c0[k] + 0.5f);
    r[k] = (uint8_t)min(max(v, 0), 255);
  }
}

template <class Tex>
__global__ void __launch_bounds__(RT_THREADS) resolve_kernel(const unsigned long long* __restrict__ pkeys,
                                                             const unsigned long long* __restrict__ tkeys, const uint8_t* __restrict__ rgb,
                                                             const uint8_t* __restrict__ rgba, int W, int H, int flipped,
                                                             uint8_t* __restrict__ out, const Tex tx, Cam c) {
  const int64_t total = (int64_t)W * H;
  for (int64_t o = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * RT_THREADS) {
    int64_t src = o;
    if (flipped) {                               // output [W][H] = the render [H][W] rotated -90 degrees: out[i][j] = render[H-1-j][i]
      const int64_t i = o / H, j = o % H;
      src = (H - 1 - j) * W + i;
    }
    const unsigned long long pk = pkeys[src], tk = tkeys[src];
    uint8_t r[3];
    if constexpr (Tex::enabled) {
      if (tk != ~0ull && (uint32_t)(tk & 0xffffffffull) >= tx.id0) {   // a textured triangle: the opaque texel replaces the point
        shade_textured(tx, c, (int)((uint32_t)(tk & 0xffffffffull) - tx.id0), (int)(src % W), (int)(src / W), r);
        out[3 * o] = r[0]; out[3 * o + 1] = r[1]; out[3 * o + 2] = r[2];
        continue;
      }
    }
    double c1[3] = {0.0, 0.0, 0.0};
    if (pk != ~0ull) {
      const int64_t p = (int64_t)(pk & 0xffffffffull);
      c1[0] = rgb[3 * p]; c1[1] = rgb[3 * p + 1]; c1[2] = rgb[3 * p + 2];
    }
    if (tk != ~0ull) {
      const int64_t t = (int64_t)(tk & 0xffffffffull);
      const double mask = (double)rgba[4 * t + 3] / 255.0;
      const double keep = 1.0 - mask;
      for (int k = 0; k < 3; ++k) {
        const double b = (double)rgba[4 * t + k] * mask + c1[k] * keep;
        r[k] = (uint8_t)(int)b;                  // numpy's astype('uint8') of a value in [0, 255]: truncation
      }
    } else {
      for (int k = 0; k < 3; ++k) r[k] = (uint8_t)(int)c1[k];
    }
    out[3 * o] = r[0]; out[3 * o + 1] = r[1]; out[3 * o + 2] = r[2];
  }
}

// one level of a mip chain from the one before: (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2x, 2y), clamped to the last
// column / row of the source (a source 1 texel wide or high)
__global__ void __launch_bounds__(RT_THREADS) mip_level_kernel(const uint8_t* __restrict__ src, int sw, int sh, uint8_t* __restrict__ dst,
                                                               int dw, int dh) {
  const int64_t total = (int64_t)dw * dh;
  for (int64_t o = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * RT_THREADS) {
    const int x = (int)(o % dw), y = (int)(o / dw);
    const int x0 = 2 * x, x1 = min(2 * x + 1, sw - 1), y0 = 2 * y, y1 = min(2 * y + 1, sh - 1);
    const uint8_t* a = src + 3 * ((int64_t)y0 * sw + x0);
    const uint8_t* b = src + 3 * ((int64_t)y0 * sw + x1);
    const uint8_t* c = src + 3 * ((int64_t)y1 * sw + x0);
    const uint8_t* d = src + 3 * ((int64_t)y1 * sw + x1);
    for (int k = 0; k < 3; ++k) dst[3 * o + k] = (uint8_t)(((int)a[k] + (int)b[k] + (int)c[k] + (int)d[k] + 2) >> 2);
  }
}

int grid_for(int64_t items, int64_t per_block) {
  const int64_t b = (items + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int acez_render_camera(const double* cam_to_world, float znear, float zfar, int width, int height, float* out_w2c12,
                                  float* out_focal) {
  ACEZ_REQUIRE(cam_to_world && out_w2c12 && out_focal, "null pointer");
  ACEZ_REQUIRE(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "frame size out of range (1 .. 16384 px per side)");
  ACEZ_REQUIRE(znear > 0.0f && zfar > znear && isfinite(zfar), "need 0 < znear < zfar < inf");
  for (int k = 0; k < 16; ++k) ACEZ_REQUIRE(isfinite(cam_to_world[k]), "camera pose is not finite");
  // rigid inverse [R^T | -R^T t] in double, then rounded to float32 once
  const double* T = cam_to_world;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) out_w2c12[4 * i + j] = (float)T[4 * j + i];
    out_w2c12[4 * i + 3] = (float)(-((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]));
  }
  *out_focal = (float)(0.5 * (double)height * 1.7320508075688772);   // yfov = pi/3: f = (H/2) / tan(pi/6) = (H/2) * sqrt(3)
  return ACEZ_OK;
}

extern "C" int acez_render_texture_size(int width, int height, int* out_levels, int64_t* out_bytes) {
  ACEZ_REQUIRE(out_levels && out_bytes, "null pointer");
  ACEZ_REQUIRE(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "texture size out of range (1 .. 16384 px per side)");
  int levels = 1;
  int64_t bytes = 0;
  for (int w = width, h = height;; ++levels) {
    bytes += (int64_t)w * h * 3;
    if (w == 1 && h == 1) break;
    w = w > 1 ? w >> 1 : 1;
    h = h > 1 ? h >> 1 : 1;
  }
  *out_levels = levels;
  *out_bytes = bytes;
  return ACEZ_OK;
}

extern "C" int acez_render_texture_build(const uint8_t* d_image, int width, int height, uint8_t* d_chain, int64_t chain_bytes, void* stream) {
  ACEZ_REQUIRE(d_image && d_chain, "null pointer");
  int levels = 0;
  int64_t bytes = 0;
  if (int rc = acez_render_texture_size(width, height, &levels, &bytes)) return rc;
  ACEZ_REQUIRE(chain_bytes >= bytes, "mip chain buffer too small (see acez_render_texture_size)");
  if (int rc = acez::require_device("rendering runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  ACEZ_HIP_CHECK(hipMemcpyAsync(d_chain, d_image, (size_t)width * height * 3, hipMemcpyDeviceToDevice, s));
  uint8_t* src = d_chain;
  for (int k = 1, sw = width, sh = height; k < levels; ++k) {
    const int dw = sw > 1 ? sw >> 1 : 1, dh = sh > 1 ? sh >> 1 : 1;
    uint8_t* dst = src + (int64_t)sw * sh * 3;
    hipLaunchKernelGGL(mip_level_kernel, dim3(grid_for((int64_t)dw * dh, RT_THREADS)), dim3(RT_THREADS), 0, s, (const uint8_t*)src, sw, sh,
                       dst, dw, dh);
    ACEZ_HIP_CHECK(hipGetLastError());
    src = dst;
    sw = dw;
    sh = dh;
  }
  return ACEZ_OK;
}

extern "C" int acez_render_frame_tex(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_tri_xyz,
                                     const uint8_t* d_tri_rgba, int64_t n_tris, const acez_tex_triangle* tex_tris, int n_tex_tris,
                                     const acez_texture* textures, int n_textures, const uint8_t* d_texels, int64_t texel_bytes,
                                     const double* cam_to_world, float znear, float zfar, int width, int height, int flipped_portrait,
                                     unsigned long long* d_work, uint8_t* d_frame, void* stream) {
  ACEZ_REQUIRE(d_work && d_frame, "null pointer");
  ACEZ_REQUIRE(n_points >= 0 && n_points < (int64_t)0xffffffff, "point count out of range (0 .. 2^32 - 2)");
  ACEZ_REQUIRE(n_tris >= 0 && n_tris < (int64_t)0xffffffff, "triangle count out of range (0 .. 2^32 - 2)");
  ACEZ_REQUIRE(n_points == 0 || (d_xyz && d_rgb), "points without coordinates or colours");
  ACEZ_REQUIRE(n_tris == 0 || (d_tri_xyz && d_tri_rgba), "triangles without vertices or colours");
  ACEZ_REQUIRE(n_tex_tris >= 0 && n_tex_tris <= ACEZ_RENDER_MAX_TEX_TRIANGLES, "textured triangle count out of range (0 .. 32)");
  ACEZ_REQUIRE(n_tris + n_tex_tris < (int64_t)0xffffffff, "triangle count out of range (0 .. 2^32 - 2)");
  ACEZ_REQUIRE(n_textures >= 0 && n_textures <= ACEZ_RENDER_MAX_TEXTURES, "texture count out of range (0 .. 16)");
  ACEZ_REQUIRE(n_tex_tris == 0 || tex_tris, "textured triangles: null pointer");
  ACEZ_REQUIRE(n_textures == 0 || (textures && d_texels), "textures: null table or texel pointer");
  TexArgs tx{};
  for (int i = 0; i < n_textures; ++i) {
    const acez_texture& t = textures[i];
    int levels = 0;
    int64_t bytes = 0;
    if (int rc = acez_render_texture_size(t.width, t.height, &levels, &bytes)) return rc;
    ACEZ_REQUIRE(t.offset >= 0 && t.offset <= texel_bytes - bytes, "texture chain outside the texel block");
    tx.tex[i] = t;
  }
  for (int i = 0; i < n_tex_tris; ++i) {
    const acez_tex_triangle& t = tex_tris[i];
    ACEZ_REQUIRE(t.texture >= 0 && t.texture < n_textures, "texture index out of range");
    for (int k = 0; k < 3; ++k) ACEZ_REQUIRE(isfinite(t.uv[k][0]) && isfinite(t.uv[k][1]), "texture coordinates are not finite");
    tx.tri[i] = t;
  }
  tx.texels = d_texels;
  tx.n = n_tex_tris;
  tx.id0 = (uint32_t)n_tris;
  Cam c{};
  if (int rc = acez_render_camera(cam_to_world, znear, zfar, width, height, c.m, &c.f)) return rc;
  c.cx = 0.5f * (float)width;
  c.cy = 0.5f * (float)height;
  c.znear = znear;
  c.zfar = zfar;
  c.W = width;
  c.H = height;
  if (int rc = acez::require_device("rendering runs on a gfx950 GPU")) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t px = (int64_t)width * height;
  unsigned long long* pkeys = d_work;
  unsigned long long* tkeys = d_work + px;
  ACEZ_HIP_CHECK(hipMemsetAsync(d_work, 0xff, (size_t)(2 * px) * sizeof(unsigned long long), s));
  if (n_points > 0) {
    hipLaunchKernelGGL(splat_points_kernel, dim3(grid_for(n_points, RT_THREADS)), dim3(RT_THREADS), 0, s, d_xyz, n_points, c, pkeys);
    ACEZ_HIP_CHECK(hipGetLastError());
  }
  if (n_tris > 0) {
    hipLaunchKernelGGL(raster_triangles_kernel, dim3(grid_for(n_tris, RT_THREADS / 64)), dim3(RT_THREADS), 0, s, d_tri_xyz, n_tris, c, tkeys);
    ACEZ_HIP_CHECK(hipGetLastError());
  }
  if (n_tex_tris > 0) {
    hipLaunchKernelGGL(raster_textured_kernel, dim3(grid_for(n_tex_tris, RT_THREADS / 64)), dim3(RT_THREADS), 0, s, tx, c, tkeys);
    ACEZ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resolve_kernel<TexArgs>, dim3(grid_for(px, RT_THREADS)), dim3(RT_THREADS), 0, s, (const unsigned long long*)pkeys,
                       (const unsigned long long*)tkeys, d_rgb, d_tri_rgba, width, height, flipped_portrait ? 1 : 0, d_frame, tx, c);
  } else {
    hipLaunchKernelGGL(resolve_kernel<NoTex>, dim3(grid_for(px, RT_THREADS)), dim3(RT_THREADS), 0, s, (const unsigned long long*)pkeys,
                       (const unsigned long long*)tkeys, d_rgb, d_tri_rgba, width, height, flipped_portrait ? 1 : 0, d_frame, NoTex{}, c);
  }
  ACEZ_HIP_CHECK(hipGetLastError());
  return ACEZ_OK;
}

extern "C" int acez_render_frame(const float* d_xyz, const uint8_t* d_rgb, int64_t n_points, const float* d_tri_xyz,
                                 const uint8_t* d_tri_rgba, int64_t n_tris, const double* cam_to_world, float znear, float zfar, int width,
                                 int height, int flipped_portrait, unsigned long long* d_work, uint8_t* d_frame, void* stream) {
  return acez_render_frame_tex(d_xyz, d_rgb, n_points, d_tri_xyz, d_tri_rgba, n_tris, nullptr, 0, nullptr, 0, nullptr, 0, cam_to_world,
                               znear, zfar, width, height, flipped_portrait, d_work, d_frame, stream);
}
