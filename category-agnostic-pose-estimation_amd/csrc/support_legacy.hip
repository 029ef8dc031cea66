// support_legacy.hip -- pieces of the reference's default support encoder (SupportPoseGraphEncoder,
// models/support_encoder.py) that are not plain GEMM / LayerNorm / attention:
//   coordinate embedding  h = relu(coords W0^T + b0)                         (first layer of coord_embedding)
//   edge info             edge_info[r] = edge_embedding[deg > 0] * max(deg, 1) / 10, deg = row sum of the skeleton adjacency
//   PE + dropout          out = dropout(x + pe[p])                            (PositionalEncoding1D.forward)
// Every reduction over rows runs in a fixed order inside one block (no float atomics): eager and replayed runs are bitwise equal.
#include "common.h"

namespace {

constexpr int LMAXP = 256;               // keypoints per graph (adjacency bitset in LDS: 256 rows x 8 words)
constexpr int LWORDS = LMAXP / 32;

__global__ void __launch_bounds__(256) legacy_coord_embed_fwd_kernel(const float* __restrict__ coords, const float* __restrict__ W0,
                                                                     const float* __restrict__ b0, float* __restrict__ h, long long R,
                                                                     int C) {
  const long long r = blockIdx.x;
  const float x = coords[r * 2 + 0], y = coords[r * 2 + 1];
  for (int c = threadIdx.x; c < C; c += blockDim.x) h[r * C + c] = fmaxf(x * W0[c * 2 + 0] + y * W0[c * 2 + 1] + b0[c], 0.f);
}

// dW0 (C, 2) += sum_r g[r][c] * coords[r], db0 += sum_r g[r][c] with g = d_h gated by relu.  One block per 64 channels,
// 16 waves (lane = channel) take every 16th row; the partial sums meet in LDS in a fixed order.
__global__ void __launch_bounds__(1024) legacy_coord_embed_wgrad_kernel(const float* __restrict__ d_h, const float* __restrict__ h,
                                                                        const float* __restrict__ coords, float* __restrict__ dW0,
                                                                        float* __restrict__ db0, long long R, int C) {
  __shared__ float part[16][3][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float gx = 0.f, gy = 0.f, gb = 0.f;
  if (c < C)
    for (long long r = w; r < R; r += 16) {
      const float g = h[r * C + c] > 0.f ? d_h[r * C + c] : 0.f;
      gx += g * coords[r * 2 + 0];
      gy += g * coords[r * 2 + 1];
      gb += g;
    }
  part[w][0][lane] = gx; part[w][1][lane] = gy; part[w][2][lane] = gb;
  __syncthreads();
  if (w == 0 && c < C) {
    float sx = 0.f, sy = 0.f, sb = 0.f;
    for (int q = 0; q < 16; ++q) { sx += part[q][0][lane]; sy += part[q][1][lane]; sb += part[q][2][lane]; }
    dW0[c * 2 + 0] += sx;
    dW0[c * 2 + 1] += sy;
    db0[c] += sb;
  }
}

// d coords[r] = sum_c g[r][c] W0[c] : one wave per row
__global__ void __launch_bounds__(256) legacy_coord_embed_dx_kernel(const float* __restrict__ d_h, const float* __restrict__ h,
                                                                    const float* __restrict__ W0, float* __restrict__ d_coords,
                                                                    long long R, int C) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                                         // wave-uniform
  const int lane = threadIdx.x & 63;
  float sx = 0.f, sy = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float g = h[r * C + c] > 0.f ? d_h[r * C + c] : 0.f;
    sx += g * W0[c * 2 + 0];
    sy += g * W0[c * 2 + 1];
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  if (lane == 0) { d_coords[r * 2 + 0] = sx; d_coords[r * 2 + 1] = sy; }
}

// One block per graph.  Edge (s, d): index s - 1 if s > 0 else s (likewise d), kept when both lie in [0, P); set symmetrically
// in an LDS bitset, so duplicates, reversed duplicates and a self-loop count once.  deg = popcount of the row.
//   out[r][c] (row stride ldo) = E[deg > 0][c] * max(deg, 1) / 10 ; scale[r] = max(deg, 1) / 10 ; has[r] = deg > 0 ; deg_out[r] = deg
__global__ void __launch_bounds__(256) legacy_edge_info_fwd_kernel(const int* __restrict__ edges, const int* __restrict__ edge_start,
                                                                   const float* __restrict__ E, float* __restrict__ out, long long ldo,
                                                                   float* __restrict__ scale, uint8_t* __restrict__ has,
                                                                   float* __restrict__ deg_out, int P, int C) {
  __shared__ uint32_t adj[LMAXP * LWORDS];
  __shared__ float sc[LMAXP];
  __shared__ int hs[LMAXP];
  const int n = blockIdx.x;
  const int W = (P + 31) >> 5;
  for (int i = threadIdx.x; i < P * W; i += blockDim.x) adj[i] = 0u;
  __syncthreads();
  for (int e = edge_start[n] + threadIdx.x; e < edge_start[n + 1]; e += blockDim.x) {
    int s = edges[2 * e], d = edges[2 * e + 1];
    s = s > 0 ? s - 1 : s;
    d = d > 0 ? d - 1 : d;
    if (s >= 0 && s < P && d >= 0 && d < P) {
      atomicOr(&adj[s * W + (d >> 5)], 1u << (d & 31));
      atomicOr(&adj[d * W + (s >> 5)], 1u << (s & 31));
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    int deg = 0;
    for (int w = 0; w < W; ++w) deg += __popc(adj[i * W + w]);
    const float s = fmaxf((float)deg, 1.f) / 10.f;
    sc[i] = s;
    hs[i] = deg > 0;
    const long long r = (long long)n * P + i;
    scale[r] = s;
    has[r] = deg > 0 ? 1 : 0;
    if (deg_out) deg_out[r] = (float)deg;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < P * C; idx += blockDim.x) {
    const int i = idx / C, c = idx - i * C;
    out[((long long)n * P + i) * ldo + c] = E[hs[i] * C + c] * sc[i];
  }
}

// dE[k][c] += sum over rows with has == k of g[r][c] * scale[r]: one block per 64 channels, 16 waves, fixed-order LDS sum
__global__ void __launch_bounds__(1024) legacy_edge_info_bwd_kernel(const float* __restrict__ g, long long ldg,
                                                                    const float* __restrict__ scale, const uint8_t* __restrict__ has,
                                                                    float* __restrict__ dE, long long R, int C) {
  __shared__ float part[16][2][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f;
  if (c < C)
    for (long long r = w; r < R; r += 16) {
      const float v = g[r * ldg + c] * scale[r];
      if (has[r]) a1 += v; else a0 += v;
    }
  part[w][0][lane] = a0; part[w][1][lane] = a1;
  __syncthreads();
  if (w == 0 && c < C) {
    float s0 = 0.f, s1 = 0.f;
    for (int q = 0; q < 16; ++q) { s0 += part[q][0][lane]; s1 += part[q][1][lane]; }
    dE[c] += s0;
    dE[C + c] += s1;
  }
}

// out[r][c] = keep(r*C + c) ? (x[r][c] + pe[r % P][c]) / (1 - p) : 0   (out may alias x)
__global__ void __launch_bounds__(256) legacy_pe_dropout_fwd_kernel(const float* x, const float* __restrict__ pe, float* out,
                                                                    long long total, int P, int C, uint32_t thresh, float inv_keep,
                                                                    const uint64_t* __restrict__ rng_state, uint32_t rng_stream) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long r = idx / C;
  const int c = (int)(idx - r * C), p_ = (int)(r % P);
  float v = x[idx] + pe[(long long)p_ * C + c];
  if (thresh) v = cape_keep(rng_state[0], rng_state[1], rng_stream, (uint64_t)idx, thresh) ? v * inv_keep : 0.f;
  out[idx] = v;
}

__global__ void __launch_bounds__(256) legacy_pe_dropout_bwd_kernel(const float* __restrict__ g, float* __restrict__ dx, long long total,
                                                                    uint32_t thresh, float inv_keep, const uint64_t* __restrict__ rng_state,
                                                                    uint32_t rng_stream) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  dx[idx] = cape_keep(rng_state[0], rng_state[1], rng_stream, (uint64_t)idx, thresh) ? g[idx] * inv_keep : 0.f;
}

}  // namespace

extern "C" int cape_legacy_coord_embed_fwd(const float* coords, const float* W0, const float* b0, float* h, int R, int C,
                                           cape_stream_t stream) {
  CAPE_REQUIRE(coords && W0 && b0 && h, "cape_legacy_coord_embed_fwd: null pointer");
  CAPE_REQUIRE(C >= 1 && R >= 0, "cape_legacy_coord_embed_fwd: bad shape");
  if (R == 0) return 0;
  hipLaunchKernelGGL(legacy_coord_embed_fwd_kernel, dim3((unsigned)R), dim3(256), 0, as_stream(stream), coords, W0, b0, h,
                     (long long)R, C);
  CAPE_LAUNCH_CHECK("cape_legacy_coord_embed_fwd");
  return 0;
}

extern "C" int cape_legacy_coord_embed_bwd(const float* d_h, const float* h, const float* coords, const float* W0, float* dW0,
                                           float* db0, float* d_coords, int R, int C, cape_stream_t stream) {
  CAPE_REQUIRE(d_h && h && coords && W0, "cape_legacy_coord_embed_bwd: null pointer");
  CAPE_REQUIRE((dW0 == nullptr) == (db0 == nullptr), "cape_legacy_coord_embed_bwd: dW0 and db0 go together");
  CAPE_REQUIRE(C >= 1 && R >= 0, "cape_legacy_coord_embed_bwd: bad shape");
  if (R == 0) return 0;
  if (dW0) {
    hipLaunchKernelGGL(legacy_coord_embed_wgrad_kernel, dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, as_stream(stream), d_h, h,
                       coords, dW0, db0, (long long)R, C);
    CAPE_LAUNCH_CHECK("cape_legacy_coord_embed_bwd(wgrad)");
  }
  if (d_coords) {
    hipLaunchKernelGGL(legacy_coord_embed_dx_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, as_stream(stream), d_h, h, W0,
                       d_coords, (long long)R, C);
    CAPE_LAUNCH_CHECK("cape_legacy_coord_embed_bwd(dx)");
  }
  return 0;
}

extern "C" int cape_support_edge_info_fwd(const int* edges, const int* edge_start, const float* E, float* out, long long ldo,
                                          float* scale, uint8_t* has, float* deg, int N, int P, int C, cape_stream_t stream) {
  CAPE_REQUIRE(edges && edge_start && E && out && scale && has, "cape_support_edge_info_fwd: null pointer");
  CAPE_REQUIRE(P >= 1 && P <= LMAXP && C >= 1 && ldo >= C && N >= 0, "cape_support_edge_info_fwd: need 1 <= P <= %d, ldo >= C",
               LMAXP);
  if (N == 0) return 0;
  hipLaunchKernelGGL(legacy_edge_info_fwd_kernel, dim3((unsigned)N), dim3(256), 0, as_stream(stream), edges, edge_start, E, out, ldo,
                     scale, has, deg, P, C);
  CAPE_LAUNCH_CHECK("cape_support_edge_info_fwd");
  return 0;
}

extern "C" int cape_support_edge_info_bwd(const float* g, long long ldg, const float* scale, const uint8_t* has, float* dE, int R,
                                          int C, cape_stream_t stream) {
  CAPE_REQUIRE(g && scale && has && dE, "cape_support_edge_info_bwd: null pointer");
  CAPE_REQUIRE(C >= 1 && ldg >= C && R >= 0, "cape_support_edge_info_bwd: bad shape");
  if (R == 0) return 0;
  hipLaunchKernelGGL(legacy_edge_info_bwd_kernel, dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, as_stream(stream), g, ldg, scale,
                     has, dE, (long long)R, C);
  CAPE_LAUNCH_CHECK("cape_support_edge_info_bwd");
  return 0;
}

extern "C" int cape_pe_dropout_fwd(const float* x, const float* pe, float* out, int R, int P, int C, float dropout_p,
                                   const uint64_t* rng_state, uint32_t rng_stream, cape_stream_t stream) {
  CAPE_REQUIRE(x && pe && out, "cape_pe_dropout_fwd: null pointer");
  CAPE_REQUIRE(R >= 0 && P >= 1 && C >= 1, "cape_pe_dropout_fwd: bad shape");
  CAPE_REQUIRE(dropout_p == 0.f || (rng_state && dropout_p > 0.f && dropout_p < 1.f), "cape_pe_dropout_fwd: dropout needs rng_state");
  const long long total = (long long)R * C;
  if (total == 0) return 0;
  const uint32_t th = dropout_p > 0.f ? cape_drop_threshold(dropout_p) : 0u;
  const float inv = dropout_p > 0.f ? 1.f / (1.f - dropout_p) : 1.f;
  hipLaunchKernelGGL(legacy_pe_dropout_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, pe, out,
                     total, P, C, th, inv, rng_state, rng_stream);
  CAPE_LAUNCH_CHECK("cape_pe_dropout_fwd");
  return 0;
}

extern "C" int cape_pe_dropout_bwd(const float* g, float* dx, long long total, float dropout_p, const uint64_t* rng_state,
                                   uint32_t rng_stream, cape_stream_t stream) {
  CAPE_REQUIRE(g && dx && rng_state, "cape_pe_dropout_bwd: null pointer");
  CAPE_REQUIRE(dropout_p > 0.f && dropout_p < 1.f && total >= 0, "cape_pe_dropout_bwd: needs 0 < p < 1");
  if (total == 0) return 0;
  hipLaunchKernelGGL(legacy_pe_dropout_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), g, dx, total,
                     cape_drop_threshold(dropout_p), 1.f / (1.f - dropout_p), rng_state, rng_stream);
  CAPE_LAUNCH_CHECK("cape_pe_dropout_bwd");
  return 0;
}
