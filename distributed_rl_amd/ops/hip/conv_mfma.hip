// Hand-written CDNA4 (gfx950) implicit-GEMM direct convolutions for the
// Atari conv stacks — NHWC, bf16 (optionally fused uint8
// dequant on the first layer), fused bias + ReLU epilogue.
//
// Replaces MIOpen igemm kernels for the fixed geometries of cfg/ape_x.json
// and cfg/impala.json (plus their R2D2 twin). Design:
//   * GEMM view: out[M=N*P*Q rows][COUT cols] = im2col(in)[M][K] x W[K][COUT],
//     K = KH*KW*C. MFMA v_mfma_f32_16x16x32_bf16, one wave computes a
//     16-row x COUT-col strip; a block = 4 waves = 64 rows.
//   * Weights (K x COUT, stored as W[cout][k] row-major = torch NHWC
//     weight.permute) are staged once into LDS as [cout][K+PAD] so B
//     fragments are ds_read_b128 with a conflict-breaking pad.
//   * A (im2col rows) is read straight from global: in NHWC every 32-wide
//     K-chunk of a patch row is 64 contiguous bytes (requires
//     (KW*C) % 32 == 0, true for all five shapes) -> one 16 B load per
//     lane per chunk; overlapping patches hit L2.
//   * Epilogue: bias + ReLU in f32, pack to bf16, scalar stores (outputs
//     are small).
//
// MFMA fragment maps (v_mfma_f32_16x16x32_bf16, guide §3):
//   A: lane l holds A[row=l&15][k=(l>>4)*8 + j], j=0..7
//   B: lane l holds B[k=(l>>4)*8 + j][col=l&15]
//   C/D: lane l holds C[row=(l>>4)*4 + r][col=l&15], r=0..3

#include <hip/hip_runtime.h>
#include <atomic>
#include <tuple>
#include <hip/hip_bf16.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int kPad = 32;  // LDS row pad: (K+pad)*2 % 256 in {64,192} spreads the
// b128 16-lane service quads across all 16 bank-row slots (PMC-verified)

template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8IN>
struct ConvGeom {
  static constexpr int P = (H - KH) / S + 1;
  static constexpr int Q = (W - KW) / S + 1;
  static constexpr int K = KH * KW * C;
  static constexpr int KCHUNKS = K / 32;
  static_assert(K % 32 == 0, "K must be a multiple of 32");
  static_assert((KW * C) % 32 == 0, "patch row must tile by 32");
  static constexpr int ROWC = KW * C;          // elements per (kh) patch row
  static constexpr int LDS_ROW = K + kPad;     // per-cout LDS stride
  static constexpr int LDS_ELEMS = COUT * LDS_ROW;
};

// A block = WAVES waves, each computing RPW rows x COUT cols
// (RPW/16 row-fragments; B fragments shared across row-fragments).
// CHW_OUT: write the output pre-flattened in logical-NCHW element order
// ((n, c*P*Q + p*Q + q)) so the trailing torch.flatten of the conv stack
// becomes a free view instead of a channels_last->NCHW copy (measured
// 8.6 us x 3 forwards per Ape-X step).
template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8IN,
          int WAVES, int RPW, bool CHW_OUT = false>
__device__ __forceinline__ void conv_fwd_block(
    const void* __restrict__ in_v,       // (N,H,W,C) u8 or bf16 (NHWC)
    const __bf16* __restrict__ weight,   // (COUT, K) row-major NHWC flat
    const __bf16* __restrict__ bias,     // (COUT), may be null
    __bf16* __restrict__ out,            // (N,P,Q,COUT)
    int batch, int tile, __bf16* wlds) {
  using G = ConvGeom<H, W, C, KH, KW, S, COUT, U8IN>;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // ---- stage weights into LDS: [cout][K + pad] ----
  constexpr int WELEMS = COUT * G::K;
  for (int base = tid * 8; base < WELEMS; base += WAVES * 64 * 8) {
    int co = base / G::K;
    int k = base - co * G::K;
    bf16x8 v = *reinterpret_cast<const bf16x8*>(weight + co * G::K + k);
    *reinterpret_cast<bf16x8*>(wlds + co * G::LDS_ROW + k) = v;
  }
  __syncthreads();

  const int M = batch * G::P * G::Q;
  const int row0 = (tile * WAVES + wave) * RPW;
  if (row0 >= M) return;
  constexpr int RFRAG = RPW / 16;
  constexpr int NFRAG = COUT / 16;
  // per-lane A row bases, one per row-fragment (clamped for ragged tail)
  int64_t in_row0[RFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    int arow = row0 + rf * 16 + (lane & 15);
    if (arow >= M) arow = M - 1;
    const int n = arow / (G::P * G::Q);
    const int rem = arow - n * (G::P * G::Q);
    const int p = rem / G::Q;
    const int q = rem - p * G::Q;
    in_row0[rf] = ((int64_t)n * H + p * S) * (W * C) + q * S * C;
  }
  const int kpart = (lane >> 4) * 8;

  f32x4 acc[RFRAG][NFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf)
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) acc[rf][f] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int kc = 0; kc < G::KCHUNKS; ++kc) {
    const int kelem = kc * 32 + kpart;
    const int dy = kelem / G::ROWC;
    const int dx = kelem - dy * G::ROWC;
    const int64_t koff = (int64_t)dy * (W * C) + dx;
    bf16x8 a[RFRAG];
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) {
      const int64_t goff = in_row0[rf] + koff;
      if constexpr (U8IN) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(in_v) + goff;
        uint2 raw = *reinterpret_cast<const uint2*>(src);
        const float inv255 = 1.0f / 255.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unsigned byte =
              (j < 4 ? raw.x >> (8 * j) : raw.y >> (8 * (j - 4))) & 0xFF;
          a[rf][j] = (__bf16)(byte * inv255);
        }
      } else {
        a[rf] = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const __bf16*>(in_v) + goff);
      }
    }
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const int col = f * 16 + (lane & 15);
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          wlds + col * G::LDS_ROW + kc * 32 + kpart);
#pragma unroll
      for (int rf = 0; rf < RFRAG; ++rf)
        acc[rf][f] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rf], b, acc[rf][f], 0, 0, 0);
    }
  }

  // ---- epilogue: bias + ReLU + bf16 store ----
  const int crow_base = (lane >> 4) * 4;
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf)
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const int col = f * 16 + (lane & 15);
      const float bv = bias ? (float)bias[col] : 0.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = row0 + rf * 16 + crow_base + r;
        if (orow < M) {
          float v = acc[rf][f][r] + bv;
          v = v > 0.0f ? v : 0.0f;
          if constexpr (CHW_OUT) {
            const int n = orow / (G::P * G::Q);
            const int pq = orow - n * (G::P * G::Q);
            out[((int64_t)n * COUT + col) * (G::P * G::Q) + pq] = (__bf16)v;
          } else {
            out[(int64_t)orow * COUT + col] = (__bf16)v;
          }
        }
      }
    }
}

template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8IN,
          int WAVES, int RPW, bool CHW_OUT = false>
__global__ __launch_bounds__(WAVES * 64) void conv_fwd_kernel(
    const void* __restrict__ in_v, const __bf16* __restrict__ weight,
    const __bf16* __restrict__ bias, __bf16* __restrict__ out, int batch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  conv_fwd_block<H, W, C, KH, KW, S, COUT, U8IN, WAVES, RPW, CHW_OUT>(
      in_v, weight, bias, out, batch, blockIdx.x,
      reinterpret_cast<__bf16*>(smem));
}

// Grouped forward: up to kMaxConvJobs independent {in, weight, bias, out}
// jobs of ONE geometry and batch size in a single launch. The job table
// travels by value in the kernel arguments (no device-side pointer table:
// nothing to upload, graph-replay safe). Block numbering is job-minor —
// block b runs row tile b / njobs of job b % njobs — so the blocks of
// different jobs on the same row tile are adjacent in dispatch order and
// jobs that share an input re-read it from L2. Each block runs the
// single-job body unchanged, so a job's output is bit-identical to its own
// conv_fwd launch.
constexpr int kMaxConvJobs = 4;
struct ConvJobs {
  const void* in[kMaxConvJobs];
  const __bf16* weight[kMaxConvJobs];
  const __bf16* bias[kMaxConvJobs];
  __bf16* out[kMaxConvJobs];
};

template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8IN,
          int WAVES, int RPW, bool CHW_OUT = false>
__global__ __launch_bounds__(WAVES * 64) void conv_fwd_grouped_kernel(
    const ConvJobs jobs, int njobs, int batch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tile = blockIdx.x / njobs;
  const int job = blockIdx.x - tile * njobs;
  conv_fwd_block<H, W, C, KH, KW, S, COUT, U8IN, WAVES, RPW, CHW_OUT>(
      jobs.in[job], jobs.weight[job], jobs.bias[job], jobs.out[job], batch,
      tile, reinterpret_cast<__bf16*>(smem));
}

// Layout probe: C(16,16) = A(16,32) x B(32,16) with exactly the fragment
// maps documented above — unit-tested against torch.matmul on the GPU so a
// map error fails loudly instead of silently transposing outputs.
__global__ void mfma_probe_kernel(const __bf16* __restrict__ A,
                                  const __bf16* __restrict__ B,
                                  float* __restrict__ C) {
  int lane = threadIdx.x & 63;
  bf16x8 a, b;
  int kpart = (lane >> 4) * 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = A[(lane & 15) * 32 + kpart + j];   // A[row][k]
    b[j] = B[(kpart + j) * 16 + (lane & 15)]; // B[k][col]
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    C[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
}

}  // namespace

// ===========================================================================
// Weight-grad (wrw) kernel: gw[COUT][K] = sum_m gout^T[COUT][m] * im2col[m][K]
// — the tall-skinny reduction GEMM of conv backward (MIOpen's igemm_wrw was
// the single biggest post-fusion cost, profiles/). The reduction dim is the
// sample dim m, so both operands need m-major fragments: we stage 32-sample
// chunks into LDS TRANSPOSED (scalar b16 writes, padded rows) so fragment
// reads are clean b128s, MFMA accumulates COUT x 64-kelem tiles, and each
// block writes its partial to its m-slice's fp32 plane (summed in a fixed
// order by wrw_reduce_kernel).
//   grid = (K/64 ktiles, MB m-slices); block = 4 waves; wave w owns the
//   16-kelem column block w.
// ===========================================================================

namespace {

constexpr int kPadM = 8;  // row pad (elements) for the staged tiles
// wrw partial planes are COUT*K floats = an even number of 256 B lines; one
// extra line makes the plane stride odd so planes spread over memory channels
constexpr int kPlanePad = 64;

typedef __bf16 v4bf_w __attribute__((ext_vector_type(4)));

// ds_read_tr16_b64 fragment read from a PLAIN row-major [32][NCOL+pad] tile:
// the 16-lane group transposes the 64 elements its lanes address, so with
// per-lane address base + (g*8 + (r>>2))*stride + 4*(r&3)  (g = lane>>4,
// r = lane&15) the result is exactly the MFMA operand fragment
// lane l -> elems j: tile[m = g*8 + j][col16 = r]  (j 0..3; second read at
// +4 rows gives j 4..7). Mapping verified on-GPU by tr16_probe (mode 1).
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* tile, int lane,
                                          int colblk) {
  const int g = lane >> 4, r = lane & 15;
  const __bf16* base =
      tile + (g * 8 + (r >> 2)) * STRIDE + colblk * 16 + 4 * (r & 3);
  auto* p0 = (__attribute__((address_space(3))) v4bf_w*)base;
  auto* p1 = (__attribute__((address_space(3))) v4bf_w*)(base + 4 * STRIDE);
  v4bf_w lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p0);
  v4bf_w hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p1);
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 4; ++j) { out[j] = lo[j]; out[j + 4] = hi[j]; }
  return out;
}

template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8IN>
__global__ __launch_bounds__(256) void conv_wrw_kernel(
    const void* __restrict__ in_v,      // (N,H,W,C) NHWC u8/bf16
    const __bf16* __restrict__ gout,    // (M, COUT) = NHWC grad (relu-masked)
    float* __restrict__ gw_part,        // (mblocks, COUT, K) fp32 partials
    int batch, int mblocks) {
  using G = ConvGeom<H, W, C, KH, KW, S, COUT, U8IN>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ASTRIDE = 64 + kPadM;
  constexpr int GSTRIDE = COUT + kPadM;
  __bf16* a_t = reinterpret_cast<__bf16*>(smem);          // [32][ASTRIDE]
  __bf16* g_t = a_t + 32 * ASTRIDE;                       // [32][GSTRIDE]

  const int ktile = blockIdx.x;
  const int mb = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int M = batch * G::P * G::Q;
  const int n_chunks = (M + 31) / 32;

  constexpr int CBLK = COUT / 16;
  f32x4 acc[CBLK];
#pragma unroll
  for (int cb = 0; cb < CBLK; ++cb) acc[cb] = {0.f, 0.f, 0.f, 0.f};

  // staging assignment (round 2, ROUND2_PLAN item 3): the thread halves
  // stage a_t and g_t CONCURRENTLY — threads 0-127 load 16-elem pieces of
  // the im2col chunk (16 B/lane for u8 input, 2x16 B for bf16; was
  // 8 B/lane with all 256 threads serialized behind g_t), threads 128-255
  // stage gout. A 16-piece never crosses a patch row: ROWC % 16 == 0 for
  // every geometry.
  static_assert(G::ROWC % 16 == 0, "16-elem staging piece crosses a row");
  const int sm = tid >> 2;             // sample row 0..31 (tid < 128)
  const int sk16 = (tid & 3) * 16;     // kelem piece base 0..48

  for (int mc = mb; mc < n_chunks; mc += mblocks) {
    const int m0 = mc * 32;
    if (tid < 128) {
      // ---- stage im2col chunk -> a_t[m][kelem]
      const int m = m0 + sm;
      const int mcl = m < M ? m : M - 1;
      const int n = mcl / (G::P * G::Q);
      const int rem = mcl - n * (G::P * G::Q);
      const int p = rem / G::Q;
      const int q = rem - p * G::Q;
      const int kelem = ktile * 64 + sk16;
      const int dy = kelem / G::ROWC;
      const int dx = kelem - dy * G::ROWC;
      const int64_t goff =
          ((int64_t)n * H + p * S + dy) * (W * C) + q * S * C + dx;
      bf16x8 v0, v1;
      if constexpr (U8IN) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(in_v) + goff;
        uint4 raw = *reinterpret_cast<const uint4*>(src);
        const float inv255 = 1.0f / 255.0f;
        const unsigned rw[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v0[j] = (__bf16)(((rw[j >> 2] >> (8 * (j & 3))) & 0xFF) * inv255);
          v1[j] = (__bf16)(((rw[2 + (j >> 2)] >> (8 * (j & 3))) & 0xFF)
                           * inv255);
        }
      } else {
        const __bf16* src = reinterpret_cast<const __bf16*>(in_v) + goff;
        v0 = *reinterpret_cast<const bf16x8*>(src);
        v1 = *reinterpret_cast<const bf16x8*>(src + 8);
      }
      if (m >= M) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v0[j] = (__bf16)0.0f;
          v1[j] = (__bf16)0.0f;
        }
      }
      *reinterpret_cast<bf16x8*>(a_t + sm * ASTRIDE + sk16) = v0;
      *reinterpret_cast<bf16x8*>(a_t + sm * ASTRIDE + sk16 + 8) = v1;
    } else {
      // ---- stage gout chunk -> g_t[m][cout] (coalesced, zero-padded)
      constexpr int PIECES = COUT / 8;
      for (int piece = tid - 128; piece < 32 * PIECES; piece += 128) {
        const int m = m0 + piece / PIECES;
        const int c0 = (piece % PIECES) * 8;
        bf16x8 v;
        if (m < M) {
          v = *reinterpret_cast<const bf16x8*>(gout + (int64_t)m * COUT + c0);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (__bf16)0.0f;
        }
        *reinterpret_cast<bf16x8*>(g_t + (piece / PIECES) * GSTRIDE + c0) = v;
      }
    }
    __syncthreads();
    // ---- fragments via tr16 reads + MFMA: wave w owns kelem block w
    bf16x8 bfrag = tr_frag<ASTRIDE>(a_t, lane, wave);
#pragma unroll
    for (int cb = 0; cb < CBLK; ++cb) {
      bf16x8 afrag = tr_frag<GSTRIDE>(g_t, lane, cb);
      acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag, bfrag, acc[cb],
                                                        0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: this m-slice's partial goes to its own (COUT, K) plane;
  // wrw_reduce_kernel sums the planes in a fixed order, so the result does
  // not depend on block scheduling (float atomics did: run-to-run jitter in
  // the last bit, which PER sampling amplifies into different batches)
  float* plane = gw_part + (int64_t)mb * (COUT * G::K + kPlanePad);
  const int kout = ktile * 64 + wave * 16 + (lane & 15);
#pragma unroll
  for (int cb = 0; cb < CBLK; ++cb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cout = cb * 16 + (lane >> 4) * 4 + r;
      plane[(int64_t)cout * G::K + kout] = acc[cb][r];
    }
}

// Ordered sum of the per-m-slice planes: block = 64 elements (16 lanes x
// float4) x 16 plane groups; group g adds planes g, g+16, ... in order, then
// the group sums fold in group order. The last block (bias == true launches one
// extra) folds the bias-grad partials of colsum_bf16_kernel the same way.
// OutT = float writes the fp32 workspaces; OutT = __bf16 rounds the final
// fp32 sums (round-to-nearest-even, what Tensor.to(bfloat16) does) and
// writes the bf16 gradients directly — (COUT, K) in (kh, kw, c) order IS the
// channels_last weight layout, so no cast or relayout pass follows.
// block: 0 .. e_blocks (the last one only with bias); sh4_raw: 256 float4.
template <typename OutT>
__device__ __forceinline__ void wrw_reduce_block(
    const float* __restrict__ part, int planes, int n_elem,
    OutT* __restrict__ out, const float* __restrict__ b_part, int b_planes,
    int cout, OutT* __restrict__ b_out, int block, float* sh4_raw) {
  float* sh = sh4_raw;
  const int tid = threadIdx.x;
  const int e_blocks = (n_elem + 63) / 64;
  if (block < e_blocks) {
    // 16 lanes x float4 = 64 elements; 16 plane groups (n_elem % 64 == 0)
    const int e4 = block * 64 + (tid & 15) * 4;
    const int g = tid >> 4;
    float4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    // four loads in flight per lane (the pass is latency-bound otherwise);
    // the adds stay in plane order g, g+16, g+32, ...
    const float4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int p = g; p < planes; p += 64) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int pu = p + 16 * u;
        v[u] = pu < planes ? *reinterpret_cast<const float4*>(
                                 part + (int64_t)pu * (n_elem + kPlanePad) + e4)
                           : zero;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w;
      }
    }
    float4* sh4 = reinterpret_cast<float4*>(sh4_raw);
    sh4[tid] = s;
    __syncthreads();
    if (tid < 16) {
      float4 t = sh4[tid];
      for (int k = 1; k < 16; ++k) {  // fixed fold order over the groups
        const float4 v = sh4[k * 16 + tid];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
      if constexpr (std::is_same<OutT, float>::value) {
        *reinterpret_cast<float4*>(out + e4) = t;
      } else {
        v4bf_w o = {(__bf16)t.x, (__bf16)t.y, (__bf16)t.z, (__bf16)t.w};
        *reinterpret_cast<v4bf_w*>(out + e4) = o;
      }
    }
  } else {
    // bias fold: thread (g, c) adds block partials g, g+G, ...; G = 256/cout
    const int G = 256 / cout;
    const int c = tid % cout, g = tid / cout;
    float s = 0.0f;
    for (int p = g; p < b_planes; p += G) s += b_part[p * cout + c];
    sh[tid] = s;
    __syncthreads();
    if (tid < cout) {
      float t = 0.0f;
      for (int k = 0; k < G; ++k) t += sh[k * cout + tid];
      b_out[tid] = (OutT)t;
    }
  }
}

template <typename OutT>
__global__ __launch_bounds__(256) void wrw_reduce_kernel(
    const float* __restrict__ part, int planes, int n_elem,
    OutT* __restrict__ out, const float* __restrict__ b_part, int b_planes,
    int cout, OutT* __restrict__ b_out) {
  __shared__ __attribute__((aligned(16))) float sh4_raw[256 * 4];
  wrw_reduce_block<OutT>(part, planes, n_elem, out, b_part, b_planes, cout,
                         b_out, (int)blockIdx.x, sh4_raw);
}

// The same fold for up to kMaxFoldJobs weight gradients in one launch: the
// job table travels by value (like ConvJobs), job j owns the next
// e_blocks(j) + (bias ? 1 : 0) blocks, and each block runs wrw_reduce_block
// unchanged, so a job's result has the bits of its own wrw_reduce_kernel
// launch. The folds of a backward are latency-bound gathers of 128-576
// blocks each; one launch at the end of the backward replaces one launch
// behind every layer's wrw.
constexpr int kMaxFoldJobs = 4;
template <typename OutT>
struct WrwFoldJobs {
  const float* part[kMaxFoldJobs];
  OutT* out[kMaxFoldJobs];
  const float* b_part[kMaxFoldJobs];  // null: no bias block
  OutT* b_out[kMaxFoldJobs];
  int planes[kMaxFoldJobs], n_elem[kMaxFoldJobs];
  int b_planes[kMaxFoldJobs], cout[kMaxFoldJobs];
  int end_block[kMaxFoldJobs];  // prefix of e_blocks + bias over the jobs
};

template <typename OutT>
__global__ __launch_bounds__(256) void wrw_reduce_grouped_kernel(
    const WrwFoldJobs<OutT> jobs, int njobs) {
  __shared__ __attribute__((aligned(16))) float sh4_raw[256 * 4];
  const int b = blockIdx.x;
  int job = 0;
#pragma unroll
  for (int j = 0; j < kMaxFoldJobs - 1; ++j)
    if (j + 1 < njobs && b >= jobs.end_block[j]) job = j + 1;
  const int first = job == 0 ? 0 : jobs.end_block[job - 1];
  wrw_reduce_block<OutT>(jobs.part[job], jobs.planes[job], jobs.n_elem[job],
                         jobs.out[job], jobs.b_part[job], jobs.b_planes[job],
                         jobs.cout[job], jobs.b_out[job], b - first, sh4_raw);
}

// bias grad: column sum of the (M, COUT) relu-masked gout — torch's
// strided bf16 reduce on channels_last costs ~11 us; this is one pass with
// an ordered block-level LDS reduction; each block writes its COUT partial
// sums to out[block][COUT] and wrw_reduce_kernel folds the blocks in order.
template <int COUT>
__global__ __launch_bounds__(256) void colsum_bf16_kernel(
    const __bf16* __restrict__ x, int64_t M, float* __restrict__ out) {
  // b128 loads (8 bf16/lane): COUT % 8 == 0, so a 16 B chunk never crosses a
  // row and covers columns phase..phase+7; the flat chunk stride
  // (gridDim*256*8) is a multiple of COUT, so each lane's phase is constant
  // and its 8 fp32 accumulators map to fixed columns. (Scalar 2 B loads
  // measured only ~0.5 TB/s — load-width bound.)
  typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
  __shared__ float sh[256 * 8];
  const int tid = threadIdx.x;
  const int64_t nchunk = M * COUT / 8;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + tid;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf8* __restrict__ x8 = (const bf8*)x;
  for (; i < nchunk; i += stride) {
    bf8 v = x8[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
  }
  // ordered block reduction (no float atomics: fixed summation order).
  // phase == (tid * 8) % COUT because gridDim-independent 2048 % COUT == 0,
  // so column c is held by threads t = c/8 + n * (COUT/8), slot c % 8.
#pragma unroll
  for (int j = 0; j < 8; ++j) sh[tid * 8 + j] = acc[j];
  __syncthreads();
  if (tid < COUT) {
    float s = 0.0f;
    for (int t = tid >> 3; t < 256; t += COUT / 8) s += sh[t * 8 + (tid & 7)];
    out[(int64_t)blockIdx.x * COUT + tid] = s;  // per-block partial
  }
}

// blocks of a colsum_bf16_kernel launch = rows of its b_part
constexpr int kColsumBlocks = 256;

}  // namespace

// tr16 semantics probe: fill LDS with 0..511, each lane passes base +
// per-lane offset `mode`, dump what each lane's 4 elements are.
namespace {
typedef __bf16 v4bf __attribute__((ext_vector_type(4)));
__global__ void tr16_probe_kernel(float* out, int mode) {
  __shared__ __bf16 lds[512];
  int lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < 512; i += 64) lds[i] = (__bf16)(float)i;
  __syncthreads();
  int off;
  switch (mode) {
    case 0: off = 0; break;                 // uniform base
    case 1: off = lane * 4; break;          // natural v4 stride
    case 2: off = (lane >> 4) * 64; break;  // group stride 64
    default: off = (lane & 15) * 4; break;
  }
  auto* p = (__attribute__((address_space(3))) v4bf*)(lds + off);
  v4bf v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[lane * 4 + j] = (float)v[j];
}
}  // namespace

// ===========================================================================
// Data-grad (dgrad) kernel — retires MIOpen igemm_bwd / ck grouped-bwd from
// the hot path (VERDICT r01 missing-5). GEMM view:
//   dx[M=N*H*W rows][C cols] = sum_{kh,kw} G[(n,y,x)][COUT] x Wt[COUT][C]
// where G gathers gout[n,(y-kh)/S,(x-kw)/S,:] when the tap is valid (stride
// divisibility + bounds) and zero otherwise. K = KH*KW*COUT runs in 32-wide
// chunks that never straddle taps (COUT % 32 == 0 for every geometry).
// B-operand comes from a PRE-TRANSPOSED weight tensor
//   w_t[c][(kh*KW+kw)*COUT + cout] = w[cout][(kh*KW+kw)*C + c]
// (built once per step by conv_w_transpose below, L2-resident), so both
// operands are plain 16 B/lane loads — no LDS at all.
// ===========================================================================
namespace {

template <int H, int W, int C, int KH, int KW, int S, int COUT, int WAVES,
          int RPW>
__global__ __launch_bounds__(WAVES * 64) void conv_dgrad_kernel(
    const __bf16* __restrict__ gout,  // (N,P,Q,COUT) NHWC
    const __bf16* __restrict__ w_t,   // (C, KH*KW*COUT)
    __bf16* __restrict__ dx,          // (N,H,W,C) NHWC
    int batch) {
  constexpr int P = (H - KH) / S + 1;
  constexpr int Q = (W - KW) / S + 1;
  constexpr int K = KH * KW * COUT;
  constexpr int KCHUNKS = K / 32;
  constexpr int CPT = COUT / 32;  // chunks per tap
  static_assert(COUT % 32 == 0, "chunks must not straddle taps");
  constexpr int RFRAG = RPW / 16;
  constexpr int NFRAG = C / 16;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int M = batch * H * W;
  const int row0 = (blockIdx.x * WAVES + wave) * RPW;
  if (row0 >= M) return;

  // per-row-fragment (n, y, x) of this lane's A row
  int a_n[RFRAG], a_y[RFRAG], a_x[RFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    int arow = row0 + rf * 16 + (lane & 15);
    if (arow >= M) arow = M - 1;
    a_n[rf] = arow / (H * W);
    const int rem = arow - a_n[rf] * (H * W);
    a_y[rf] = rem / W;
    a_x[rf] = rem - a_y[rf] * W;
  }
  const int kpart = (lane >> 4) * 8;

  f32x4 acc[RFRAG][NFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf)
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) acc[rf][f] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int kc = 0; kc < KCHUNKS; ++kc) {
    const int tap = kc / CPT;
    const int kh = tap / KW;
    const int kw = tap - kh * KW;
    const int co = (kc - tap * CPT) * 32 + kpart;
    bf16x8 a[RFRAG];
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) {
      const int py = a_y[rf] - kh;
      const int qx = a_x[rf] - kw;
      const int p = py / S, q = qx / S;
      const bool ok = py >= 0 && qx >= 0 && py == p * S && qx == q * S &&
                      p < P && q < Q;
      if (ok) {
        a[rf] = *reinterpret_cast<const bf16x8*>(
            gout + (((int64_t)a_n[rf] * P + p) * Q + q) * COUT + co);
      } else {
        a[rf] = bf16x8{};
      }
    }
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const int col = f * 16 + (lane & 15);
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          w_t + (int64_t)col * K + tap * COUT + co);
#pragma unroll
      for (int rf = 0; rf < RFRAG; ++rf)
        acc[rf][f] =
            __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[rf], b, acc[rf][f], 0, 0, 0);
    }
  }

  const int crow_base = (lane >> 4) * 4;
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf)
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const int col = f * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = row0 + rf * 16 + crow_base + r;
        if (orow < M) dx[(int64_t)orow * C + col] = (__bf16)acc[rf][f][r];
      }
    }
}

__global__ void conv_w_transpose_kernel(const __bf16* __restrict__ w,
                                        __bf16* __restrict__ w_t, int TAPS,
                                        int C, int COUT) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = TAPS * C * COUT;
  if (i >= total) return;
  const int co = i / (TAPS * C);
  const int rem = i - co * (TAPS * C);
  const int tap = rem / C;
  const int c = rem - tap * C;
  w_t[((int64_t)c * TAPS + tap) * COUT + co] = w[i];
}

}  // namespace

// relu-mask + CHW->NHWC transpose in one pass (backward of the fused
// flatten): masked[n,p,q,c] = gout_chw[n,c,pq] * (out_chw > 0)
namespace {
__global__ void relu_mask_bwd_chw_kernel(const __bf16* __restrict__ gout,
                                         const __bf16* __restrict__ outv,
                                         __bf16* __restrict__ dst, int64_t N,
                                         int C, int PQ) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = N * (int64_t)C * PQ;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int c = (int)(i % C);
    const int64_t t = i / C;
    const int pq = (int)(t % PQ);
    const int64_t n = t / PQ;
    const int64_t src = ((int64_t)n * C + c) * PQ + pq;
    dst[i] = ((float)outv[src] > 0.0f) ? gout[src] : (__bf16)0.0f;
  }
}
}  // namespace

// ===========================================================================
// Fused Linear(+bias)+ReLU forward for the MLP trunk head (round 2):
// out(M, N) = relu(x(M, K) @ W(N, K)^T + b). hipBLASLt runs this shape
// (512, 3136)->(1024) at ~17.6 us + a separate 5 us ReLU; this kernel
// fuses the epilogue and tiles for the chip: 64 blocks x 4 waves, each
// wave a 16-row x 128-col strip, W k-slices staged through LDS per
// 64-wide K chunk (b128 fragment reads, conflict pad).
// ===========================================================================
namespace {

template <int K, int N, int NT /*cols per block*/>
__global__ __launch_bounds__(256) void linear_relu_kernel(
    const __bf16* __restrict__ x,   // (M, K)
    const __bf16* __restrict__ w,   // (N, K)
    const __bf16* __restrict__ b,   // (N) or null
    __bf16* __restrict__ out,       // (M, N)
    int M) {
  constexpr int KB = 64;            // K chunk staged per iteration
  constexpr int LROW = KB + 32;     // (LROW*2)%256 == 192: bank-spread pad
  __shared__ __bf16 wlds[NT][LROW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  // block tile: 32 rows x NT cols; waves 2x2 over (16 rows x NT/2 cols)
  const int row0 = blockIdx.x * 32 + (wave >> 1) * 16;
  const int col0 = blockIdx.y * NT + (wave & 1) * (NT / 2);
  constexpr int NFRAG = NT / 2 / 16;
  const int arow = row0 + (lane & 15);
  const int arow_c = arow < M ? arow : (M > 0 ? M - 1 : 0);
  const int kpart = (lane >> 4) * 8;

  f32x4 acc[NFRAG];
#pragma unroll
  for (int f = 0; f < NFRAG; ++f) acc[f] = {0.f, 0.f, 0.f, 0.f};

  // software pipeline: the next chunk's W pieces are prefetched into
  // registers while the current chunk's MFMAs run (a single-buffered
  // stage->sync->MFMA loop exposed the full global latency per chunk)
  constexpr int PIECES = NT * KB / (256 * 8);
  bf16x8 wpre[PIECES];
#pragma unroll
  for (int pc = 0; pc < PIECES; ++pc) {
    const int base = (tid + pc * 256) * 8;
    const int r = base / KB;
    wpre[pc] = *reinterpret_cast<const bf16x8*>(
        w + (int64_t)(blockIdx.y * NT + r) * K + (base - r * KB));
  }
  // A fragments also 1-deep prefetched (they were the remaining serial
  // latency chain: one L2 round-trip per 16 MFMAs)
  bf16x8 a_cur[2], a_nxt[2];
#pragma unroll
  for (int kc = 0; kc < 2; ++kc)
    a_cur[kc] = *reinterpret_cast<const bf16x8*>(
        x + (int64_t)arow_c * K + kc * 32 + kpart);
  for (int k0 = 0; k0 < K; k0 += KB) {
    __syncthreads();
#pragma unroll
    for (int pc = 0; pc < PIECES; ++pc) {
      const int base = (tid + pc * 256) * 8;
      const int r = base / KB;
      *reinterpret_cast<bf16x8*>(&wlds[r][base - r * KB]) = wpre[pc];
    }
    __syncthreads();
    if (k0 + KB < K) {
#pragma unroll
      for (int kc = 0; kc < 2; ++kc)
        a_nxt[kc] = *reinterpret_cast<const bf16x8*>(
            x + (int64_t)arow_c * K + k0 + KB + kc * 32 + kpart);
    }
    if (k0 + KB < K) {
#pragma unroll
      for (int pc = 0; pc < PIECES; ++pc) {
        const int base = (tid + pc * 256) * 8;
        const int r = base / KB;
        wpre[pc] = *reinterpret_cast<const bf16x8*>(
            w + (int64_t)(blockIdx.y * NT + r) * K + k0 + KB +
            (base - r * KB));
      }
    }
#pragma unroll
    for (int kc = 0; kc < KB / 32; ++kc) {
      bf16x8 a = a_cur[kc];
#pragma unroll
      for (int f = 0; f < NFRAG; ++f) {
        const int wl = (wave & 1) * (NT / 2) + f * 16 + (lane & 15);
        bf16x8 bf = *reinterpret_cast<const bf16x8*>(
            &wlds[wl][kc * 32 + kpart]);
        acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bf, acc[f], 0, 0, 0);
      }
    }
    a_cur[0] = a_nxt[0];
    a_cur[1] = a_nxt[1];
  }
  const int crow = (lane >> 4) * 4;
#pragma unroll
  for (int f = 0; f < NFRAG; ++f) {
    const int col = col0 + f * 16 + (lane & 15);
    const float bv = b ? (float)b[col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int orow = row0 + crow + r;
      if (orow < M) {
        float v = acc[f][r] + bv;
        out[(int64_t)orow * N + col] = (__bf16)(v > 0.0f ? v : 0.0f);
      }
    }
  }
}
}  // namespace

// ===========================================================================
// 3x3 stride-1 pad-1 forward for the IMPALA-ResNet torso
// (cfg/impala_resnet.json: 84x84 input, channels 16/32/32 -> 42x42x16,
// 42x42x16->32, 21x21x32, 11x11x32). Same implicit-GEMM view, LDS-staged
// weights and 16x16x32 bf16 fragment maps as conv_fwd_kernel, plus:
//   * padding: K order is (kh, kw, c) = the channels_last weight viewed as
//     (COUT, 9C). A lane's 8-element piece lies inside one tap (8 | C):
//     tap = kelem / C, (dy, dx) = (tap/3 - 1, tap%3 - 1). A piece whose tap
//     falls outside the image (or past tap 8, C=16 tail) is exact zeros and
//     is never loaded — the address is not dereferenced.
//   * C=32: K=288 = 9 chunks, one tap each. C=16: K=144 padded to 160 in
//     LDS (columns 144..159 zero) = 5 chunks of two taps.
//   * operands swapped in the MFMA (weights as A, im2col rows as B — the
//     per-lane loads are identical since both maps are [l&15][8*(l>>4)+j]):
//     the accumulator then holds out^T, i.e. 4 consecutive couts of one
//     output row per lane -> 8-byte residual loads and output stores.
//   * fusions: relu_in on the A pieces as they are loaded; epilogue in f32:
//     + bias, + residual, ReLU (relu_out), round to bf16.
//   * MASK (compile-time; the input-gradient use below): the epilogue keeps
//     v where mask > 0 and writes 0 elsewhere, decided on the f32 value
//     before rounding — the relu_in mask of the conv whose input gradient
//     this is. mask has the output's shape. MASK=false is the forward.
// ===========================================================================
namespace {

using s16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

template <int C, int COUT>
struct Conv3Geom {
  static constexpr int K = 9 * C;
  static constexpr int KP = (K + 31) / 32 * 32;  // 288 (C=32), 160 (C=16)
  static constexpr int KCHUNKS = KP / 32;
  // row pad chosen per geometry for the kPad rule: (row_elems*2) % 256 in
  // {64, 192}. 288 and 160 both land on 64 with no pad at all.
  static constexpr int PAD = 0;
  static constexpr int LDS_ROW = KP + PAD;
  static constexpr int LDS_ELEMS = COUT * LDS_ROW;
  static constexpr int LDS_BYTES = (LDS_ELEMS + COUT) * 2;  // weights + bias
  static_assert(C % 8 == 0, "an 8-element piece must not straddle a tap");
  static_assert((LDS_ROW * 2) % 256 == 64 || (LDS_ROW * 2) % 256 == 192,
                "LDS row stride breaks the bank-spread rule");
  static_assert(LDS_ROW % 8 == 0, "LDS rows must stay 16-byte aligned");
  static_assert(COUT % 16 == 0, "COUT must tile by 16");
  static_assert(COUT <= 64, "bias staging uses the first COUT threads");
};

// The image extent of the four 3x3 pad-1 kernel bodies below (forward, wrw,
// stem forward, stem wrw). H and W occur in a body only in the row decode,
// the two bounds tests and the tap offset; tiling, LDS layout, fragment
// maps and epilogues depend on (C, COUT) alone. Two implementations:
//   * HwConst<H, W>: compile-time constants — the table kernels
//     (kConv3Launches, kStemLaunches), whose code is what it was when H and
//     W were template arguments of the body;
//   * HwArgs: two ints passed as kernel arguments — the *_hw_kernel
//     instantiations, one per (C, COUT), for every other frame size.
template <int HC, int WC>
struct HwConst {
  static constexpr int H = HC, W = WC;
};
struct HwArgs {
  int H, W;
};

template <class HW, int C, int COUT, int WAVES, int RPW, bool MASK>
__device__ __forceinline__ void conv3x3p1_fwd_body(
    const HW hw,
    const __bf16* __restrict__ in,        // (N,H,W,C) NHWC
    const __bf16* __restrict__ weight,    // (COUT, 9C) = (cout, kh, kw, c)
    const __bf16* __restrict__ bias,      // (COUT), may be null
    const __bf16* __restrict__ residual,  // (N,H,W,COUT), may be null
    const __bf16* __restrict__ mask,      // (N,H,W,COUT), MASK only
    __bf16* __restrict__ out,             // (N,H,W,COUT)
    int batch, int relu_in, int relu_out) {
  using G = Conv3Geom<C, COUT>;
  const int H = hw.H, W = hw.W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* wlds = reinterpret_cast<__bf16*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // ---- stage weights into LDS: [cout][KP + pad], K tail zero-filled ----
  for (int base = tid * 8; base < COUT * G::KP; base += WAVES * 64 * 8) {
    const int co = base / G::KP;
    const int k = base - co * G::KP;
    bf16x8 v = {};
    if (k < G::K) v = *reinterpret_cast<const bf16x8*>(weight + co * G::K + k);
    *reinterpret_cast<bf16x8*>(wlds + co * G::LDS_ROW + k) = v;
  }
  // bias rides along behind the weights (a bias living in a flat parameter
  // buffer is only 2-byte aligned: scalar loads here, one b64 read later)
  __bf16* blds = wlds + G::LDS_ELEMS;
  if (tid < COUT) blds[tid] = bias ? bias[tid] : (__bf16)0.0f;
  __syncthreads();

  const int M = batch * H * W;
  const int row0 = (blockIdx.x * WAVES + wave) * RPW;
  if (row0 >= M) return;
  constexpr int RFRAG = RPW / 16;
  constexpr int NFRAG = COUT / 16;
  // per-lane im2col row, one per row-fragment (clamped for the ragged tail)
  int64_t in_row0[RFRAG];
  int a_p[RFRAG], a_q[RFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    int arow = row0 + rf * 16 + (lane & 15);
    if (arow >= M) arow = M - 1;
    const int n = arow / (H * W);
    const int rem = arow - n * (H * W);
    a_p[rf] = rem / W;
    a_q[rf] = rem - a_p[rf] * W;
    in_row0[rf] = (int64_t)arow * C;  // ((n*H + p)*W + q)*C
  }
  const int kpart = (lane >> 4) * 8;
  const short relu_bits = relu_in ? (short)-1 : (short)0;

  f32x4 acc[RFRAG][NFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf)
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) acc[rf][f] = {0.f, 0.f, 0.f, 0.f};

  // ---- phase 1: every live A piece of the whole K range goes in flight
  // before the first use (a load-then-use per chunk serialises one L2
  // round trip per piece). Dead pieces keep their zeros; their address is
  // never formed into a load.
  s16x8 a[G::KCHUNKS][RFRAG];
#pragma unroll
  for (int kc = 0; kc < G::KCHUNKS; ++kc)
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) a[kc][rf] = s16x8{};
#pragma unroll
  for (int kc = 0; kc < G::KCHUNKS; ++kc) {
    const int kelem = kc * 32 + kpart;
    const int tap = kelem / C;
    const int c0 = kelem - tap * C;
    const int th = tap / 3;
    const int dy = th - 1;
    const int dx = tap - th * 3 - 1;
    const int64_t koff = (int64_t)(dy * W + dx) * C + c0;
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) {
      const bool live = tap < 9 && (unsigned)(a_p[rf] + dy) < (unsigned)H &&
                        (unsigned)(a_q[rf] + dx) < (unsigned)W;
      if (live)
        a[kc][rf] = *reinterpret_cast<const s16x8*>(in + in_row0[rf] + koff);
    }
  }

  // the residual goes in flight with the A pieces: 4 consecutive couts
  // per (row-fragment, col-fragment)
  const int ccol = (lane >> 4) * 4;
  bf16x4 rv[RFRAG][NFRAG];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    const int orow = row0 + rf * 16 + (lane & 15);
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      rv[rf][f] = bf16x4{};
      if (residual && orow < M)
        rv[rf][f] = *reinterpret_cast<const bf16x4*>(
            residual + (int64_t)orow * COUT + f * 16 + ccol);
    }
  }

  // the mask goes in flight with them too (bf16 bits: > 0 <=> sign clear
  // and not zero, as relu_mask_bwd decides it)
  using u16x4 = __attribute__((ext_vector_type(4))) unsigned short;
  u16x4 mv[MASK ? RFRAG : 1][MASK ? NFRAG : 1];
  if constexpr (MASK) {
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) {
      const int orow = row0 + rf * 16 + (lane & 15);
#pragma unroll
      for (int f = 0; f < NFRAG; ++f) {
        mv[rf][f] = u16x4{};
        if (orow < M)
          mv[rf][f] = *reinterpret_cast<const u16x4*>(
              mask + (int64_t)orow * COUT + f * 16 + ccol);
      }
    }
  }

  // ---- phase 2: relu_in on the bf16 bits (clear every element whose sign
  // bit is set), then the MFMAs
#pragma unroll
  for (int kc = 0; kc < G::KCHUNKS; ++kc) {
    bf16x8 av[RFRAG];
#pragma unroll
    for (int rf = 0; rf < RFRAG; ++rf) {
      const s16x8 s = a[kc][rf];
      av[rf] = __builtin_bit_cast(bf16x8, s & ~((s >> 15) & relu_bits));
    }
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const int col = f * 16 + (lane & 15);
      bf16x8 b = *reinterpret_cast<const bf16x8*>(
          wlds + col * G::LDS_ROW + kc * 32 + kpart);
#pragma unroll
      for (int rf = 0; rf < RFRAG; ++rf)
        acc[rf][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, av[rf],
                                                             acc[rf][f], 0, 0, 0);
    }
  }

  // ---- epilogue: acc[rf][f][r] = out[row0 + rf*16 + (l&15)]
  //                                   [f*16 + (l>>4)*4 + r]
  // + bias, + residual, ReLU in f32; one 8-byte store per (rf, f)
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    const int orow = row0 + rf * 16 + (lane & 15);
    if (orow >= M) continue;
#pragma unroll
    for (int f = 0; f < NFRAG; ++f) {
      const bf16x4 bv = *reinterpret_cast<const bf16x4*>(blds + f * 16 + ccol);
      bf16x4 ov;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[rf][f][r] + (float)bv[r];
        v += (float)rv[rf][f][r];
        if (relu_out) v = v > 0.0f ? v : 0.0f;
        if constexpr (MASK) {
          const unsigned short mb = mv[rf][f][r];
          if ((mb & 0x8000) || mb == 0) v = 0.0f;
        }
        ov[r] = (__bf16)v;
      }
      *reinterpret_cast<bf16x4*>(out + (int64_t)orow * COUT + f * 16 + ccol) =
          ov;
    }
  }
}

// table kernel: H and W compile-time (kConv3Launches)
template <int H, int W, int C, int COUT, int WAVES, int RPW, bool MASK = false>
__global__ __launch_bounds__(WAVES * 64) void conv3x3p1_fwd_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ weight,
    const __bf16* __restrict__ bias, const __bf16* __restrict__ residual,
    const __bf16* __restrict__ mask, __bf16* __restrict__ out, int batch,
    int relu_in, int relu_out) {
  conv3x3p1_fwd_body<HwConst<H, W>, C, COUT, WAVES, RPW, MASK>(
      HwConst<H, W>{}, in, weight, bias, residual, mask, out, batch, relu_in,
      relu_out);
}

// run-time kernel: H and W are arguments (kConv3HwLaunches)
template <int C, int COUT, int WAVES, int RPW, bool MASK = false>
__global__ __launch_bounds__(WAVES * 64) void conv3x3p1_fwd_hw_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ weight,
    const __bf16* __restrict__ bias, const __bf16* __restrict__ residual,
    const __bf16* __restrict__ mask, __bf16* __restrict__ out, int batch,
    int relu_in, int relu_out, int H, int W) {
  conv3x3p1_fwd_body<HwArgs, C, COUT, WAVES, RPW, MASK>(
      HwArgs{H, W}, in, weight, bias, residual, mask, out, batch, relu_in,
      relu_out);
}

// ---------------------------------------------------------------------------
// Weight gradient of the same convs:
//   gw[co][(kh,kw,c)] = sum_m gout[m][co] * im2col(x)[m][(kh,kw,c)], M = N*H*W
// with K in the channels_last weight order, so no relayout follows. Built on
// conv_wrw_kernel's scheme: 32-sample chunks staged plain row-major in LDS,
// tr_frag fragments, fp32 MFMA accumulate, one fp32 plane per m-slice folded
// in a fixed order by wrw_reduce_kernel (no float atomics: two calls on the
// same inputs are bit-identical). What differs:
//   * one block covers ALL of K (144 or 288 = 9 or 18 column blocks of 16),
//     so the gout chunk is staged once per chunk, not once per K-tile; the
//     staged x tile is [32][K+8] per chunk (< 19 KB). Wave w owns column blocks
//     w, w+4, ... (3/2/2/2 of 9, 5/5/4/4 of 18) against every cout block.
//   * padding as in the forward: an 8-element piece lies inside one tap and
//     is live iff its tap is inside the image; dead pieces and rows past M
//     stay zeros and their address is never formed into a load.
//   * relu_in clears the sign-bit elements of the x pieces as they are
//     staged (the forward's bit trick).
//   * a block takes R consecutive 32-sample chunks per pass and loads the
//     next pass's pieces into registers before the current pass's MFMAs.
//     More chunks per pass put more bytes in flight but cost registers and
//     LDS, i.e. resident blocks; R is picked per geometry from a
//     measurement (profiles/r06_resconv_bwd.md).
// Staging: thread t stages rows (t>>3) + 32s, pieces (t&7) + 8i of each —
// the (n, p, q) decode is once per row, and eight neighbouring lanes read
// 128 contiguous bytes.
// ---------------------------------------------------------------------------
template <int C, int COUT, int R>
struct Conv3Wrw {
  static constexpr int K = 9 * C;
  static constexpr int NCB = K / 16;         // column blocks: 9 / 18
  static constexpr int CBW = (NCB + 3) / 4;  // per wave: 3 / 5
  static constexpr int CBLK = COUT / 16;
  static constexpr int PPR = K / 8;          // x pieces per row: 18 / 36
  static constexpr int XIT = (PPR + 7) / 8;  // staging passes: 3 / 5
  static constexpr int GP = COUT / 8;        // gout pieces per row
  static constexpr int XSTRIDE = K + kPadM;
  static constexpr int GSTRIDE = COUT + kPadM;
  static constexpr int ROWS = 32 * R;        // sample rows per pass
  static constexpr int GIT = (ROWS * GP + 255) / 256;  // gout staging passes
  static constexpr int LDS_BYTES = ROWS * (XSTRIDE + GSTRIDE) * 2;
  static_assert(C % 8 == 0 && COUT % 16 == 0 && K % 16 == 0, "tiling");
  static_assert(LDS_BYTES <= 64 * 1024, "dynamic LDS limit");
  static_assert(XSTRIDE % 8 == 0 && GSTRIDE % 8 == 0, "16-byte LDS rows");
};

template <class HW, int C, int COUT, int R>
__device__ __forceinline__ void conv3x3p1_wrw_body(
    const HW hw,
    const __bf16* __restrict__ x,     // (N,H,W,C) NHWC
    const __bf16* __restrict__ gout,  // (M, COUT) = NHWC grad (relu-masked)
    float* __restrict__ gw_part,      // (mblocks, COUT*K + kPlanePad) fp32
    int batch, int mblocks, int relu_in) {
  using G = Conv3Wrw<C, COUT, R>;
  const int H = hw.H, W = hw.W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* x_t = reinterpret_cast<__bf16*>(smem);  // [ROWS][XSTRIDE]
  __bf16* g_t = x_t + G::ROWS * G::XSTRIDE;       // [ROWS][GSTRIDE]

  const int mb = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform in an SGPR: the column-block guards below must stay scalar
  // branches (tr16 reads need the whole wave active)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = batch * H * W;
  const int n_pass = (M + G::ROWS - 1) / G::ROWS;

  f32x4 acc[G::CBW][G::CBLK];
#pragma unroll
  for (int i = 0; i < G::CBW; ++i)
#pragma unroll
    for (int cb = 0; cb < G::CBLK; ++cb) acc[i][cb] = {0.f, 0.f, 0.f, 0.f};

  const int srow = tid >> 3;  // staged sample row 0..31 (+ 32s)
  const int sj = tid & 7;     // first x piece of that row
  const short relu_bits = relu_in ? (short)-1 : (short)0;

  s16x8 xr[R][G::XIT];
  s16x8 gr[G::GIT];
  auto load_pass = [&](int mc) __attribute__((always_inline)) {
    const int m0 = mc * G::ROWS;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int m = m0 + s * 32 + srow;
      const bool valid = m < M;
      const int mcl = valid ? m : 0;
      const int rem = mcl % (H * W);
      const int p = rem / W;
      const int q = rem - p * W;
      const __bf16* xrow = x + (int64_t)mcl * C;  // ((n*H + p)*W + q)*C
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        xr[s][i] = s16x8{};
        const int kp = sj + 8 * i;
        const int kelem = kp * 8;
        const int tap = kelem / C;
        const int c0 = kelem - tap * C;
        const int th = tap / 3;
        const int dy = th - 1;
        const int dx = tap - th * 3 - 1;
        const bool live = valid && kp < G::PPR &&
                          (unsigned)(p + dy) < (unsigned)H &&
                          (unsigned)(q + dx) < (unsigned)W;
        if (live)
          xr[s][i] = *reinterpret_cast<const s16x8*>(
              xrow + (int64_t)(dy * W + dx) * C + c0);
      }
    }
#pragma unroll
    for (int t = 0; t < G::GIT; ++t) {
      const int piece = tid + 256 * t;
      const int m = m0 + piece / G::GP;
      gr[t] = s16x8{};
      if (piece < G::ROWS * G::GP && m < M)
        gr[t] = *reinterpret_cast<const s16x8*>(
            gout + (int64_t)m * COUT + (piece % G::GP) * 8);
    }
  };

  if (mb < n_pass) load_pass(mb);
  for (int mc = mb; mc < n_pass; mc += mblocks) {
    // ---- registers -> LDS (relu_in on the bf16 bits)
#pragma unroll
    for (int s = 0; s < R; ++s)
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        const int kp = sj + 8 * i;
        if (kp < G::PPR) {
          const s16x8 v = xr[s][i];
          *reinterpret_cast<s16x8*>(x_t + (s * 32 + srow) * G::XSTRIDE +
                                    kp * 8) = v & ~((v >> 15) & relu_bits);
        }
      }
#pragma unroll
    for (int t = 0; t < G::GIT; ++t) {
      const int piece = tid + 256 * t;
      if (piece < G::ROWS * G::GP)
        *reinterpret_cast<s16x8*>(g_t + (piece / G::GP) * G::GSTRIDE +
                                  (piece % G::GP) * 8) = gr[t];
    }
    __syncthreads();
    if (mc + mblocks < n_pass) load_pass(mc + mblocks);
    // ---- fragments via tr16 reads + MFMA, chunk by chunk
#pragma unroll
    for (int s = 0; s < R; ++s) {
      bf16x8 gf[G::CBLK];
#pragma unroll
      for (int cb = 0; cb < G::CBLK; ++cb)
        gf[cb] = tr_frag<G::GSTRIDE>(g_t + s * 32 * G::GSTRIDE, lane, cb);
#pragma unroll
      for (int i = 0; i < G::CBW; ++i) {
        const int colblk = wave + 4 * i;
        if (colblk < G::NCB) {
          const bf16x8 xf =
              tr_frag<G::XSTRIDE>(x_t + s * 32 * G::XSTRIDE, lane, colblk);
#pragma unroll
          for (int cb = 0; cb < G::CBLK; ++cb)
            acc[i][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                gf[cb], xf, acc[i][cb], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // ---- epilogue: this m-slice's partial goes to its own (COUT, K) plane
  float* plane = gw_part + (int64_t)mb * (COUT * G::K + kPlanePad);
#pragma unroll
  for (int i = 0; i < G::CBW; ++i) {
    const int colblk = wave + 4 * i;
    if (colblk < G::NCB) {
      const int kout = colblk * 16 + (lane & 15);
#pragma unroll
      for (int cb = 0; cb < G::CBLK; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cout = cb * 16 + (lane >> 4) * 4 + r;
          plane[cout * G::K + kout] = acc[i][cb][r];
        }
    }
  }
}

template <int H, int W, int C, int COUT, int R>
__global__ __launch_bounds__(256) void conv3x3p1_wrw_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ gout,
    float* __restrict__ gw_part, int batch, int mblocks, int relu_in) {
  conv3x3p1_wrw_body<HwConst<H, W>, C, COUT, R>(HwConst<H, W>{}, x, gout,
                                                gw_part, batch, mblocks,
                                                relu_in);
}

template <int C, int COUT, int R>
__global__ __launch_bounds__(256) void conv3x3p1_wrw_hw_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ gout,
    float* __restrict__ gw_part, int batch, int mblocks, int relu_in, int H,
    int W) {
  conv3x3p1_wrw_body<HwArgs, C, COUT, R>(HwArgs{H, W}, x, gout, gw_part, batch,
                                         mblocks, relu_in);
}

// Input gradient: for a 3x3 stride-1 pad-1 conv it is itself a 3x3 stride-1
// pad-1 conv of gout with the weight transposed and flipped,
//   W'[ci][kh][kw][co] = W[co][2-kh][2-kw][ci],
// so conv3x3p1_fwd_kernel runs it at the mirrored geometry (H, W, COUT, C).
// One launch per conv writes W' (a kernel, not torch ops: the step is
// graph-captured). Tap index t = kh*3 + kw flips to 8 - t.
__global__ void conv3x3_w_flip_kernel(const __bf16* __restrict__ w,
                                      __bf16* __restrict__ w_f, int C,
                                      int COUT) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 9 * C * COUT) return;
  const int ci = i / (9 * COUT);
  const int rem = i - ci * (9 * COUT);
  const int tap = rem / COUT;
  const int co = rem - tap * COUT;
  w_f[i] = w[(co * 9 + (8 - tap)) * C + ci];
}

using Conv3Fn = void (*)(const __bf16*, const __bf16*, const __bf16*,
                         const __bf16*, const __bf16*, __bf16*, int, int, int);

// ONE entry per (H, W, C, COUT) carries every kernel of that geometry
struct Conv3Launch {
  int H, W, C, COUT;
  Conv3Fn fn;       // forward
  Conv3Fn fn_mask;  // forward with the masked epilogue (input gradients)
  int lds_bytes;
  int waves, rpw;
  // weight-grad + its bias-grad column sum (null: forward-only geometry)
  void (*wrw)(const __bf16*, const __bf16*, float*, int, int, int);
  int wrw_lds_bytes, wrw_rows;  // rows: samples a block takes per pass
  void (*colsum)(const __bf16*, int64_t, float*);
};

// WRW_R: 32-sample chunks per pass of the weight-grad (0: forward only)
template <int H, int W, int C, int COUT, int WAVES, int RPW, int WRW_R>
Conv3Launch make_conv3() {
  using G = Conv3Geom<C, COUT>;
  Conv3Launch l{};
  l.H = H; l.W = W; l.C = C; l.COUT = COUT;
  l.fn = conv3x3p1_fwd_kernel<H, W, C, COUT, WAVES, RPW, false>;
  // every geometry has its masked twin, because conv3x3p1_dgrad takes a
  // mask at every geometry; the model launches three of the five (the
  // relu_in convs are the C -> C ones; 42x42x16->32 and 42x42x32->16 run
  // masked only from the tests)
  l.fn_mask = conv3x3p1_fwd_kernel<H, W, C, COUT, WAVES, RPW, true>;
  l.lds_bytes = G::LDS_BYTES;
  l.waves = WAVES;
  l.rpw = RPW;
  if constexpr (WRW_R > 0) {
    l.wrw = conv3x3p1_wrw_kernel<H, W, C, COUT, WRW_R>;
    l.wrw_lds_bytes = Conv3Wrw<C, COUT, WRW_R>::LDS_BYTES;
    l.wrw_rows = 32 * WRW_R;
    l.colsum = colsum_bf16_kernel<COUT>;
  }
  return l;
}

// cfg/impala_resnet.json at 84x84 (the first conv, C=4 -> K=36, is not in
// this table: it has kStemLaunches and its own kernels below)
static const Conv3Launch kConv3Launches[] = {
    // WRW_R: the fastest of 1, 2, 4 per geometry at 1344 images
    // (profiles/r06_resconv_bwd.md)
    make_conv3<42, 42, 16, 16, 8, 32, 1>(),  // section-1 residual convs
    make_conv3<42, 42, 16, 32, 8, 32, 4>(),  // section-2 entry conv
    make_conv3<21, 21, 32, 32, 8, 32, 2>(),  // section-3 entry, sec-2 residual
    make_conv3<11, 11, 32, 32, 8, 16, 1>(),  // section-3 residual convs
    // input gradient of the section-2 entry conv (forward kernels only)
    make_conv3<42, 42, 32, 16, 8, 32, 0>(),
};

const Conv3Launch* find_conv3(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  for (const auto& l : kConv3Launches)
    if (l.H == H && l.W == W && l.C == C && l.COUT == COUT) return &l;
  return nullptr;
}

// The run-time entries: ONE per (C, COUT), Conv3Launch's fields with H and
// W moved from the key to two trailing kernel arguments. A geometry that
// kConv3Launches does not hold launches these.
using Conv3HwFn = void (*)(const __bf16*, const __bf16*, const __bf16*,
                           const __bf16*, const __bf16*, __bf16*, int, int,
                           int, int, int);

struct Conv3HwLaunch {
  int C, COUT;
  Conv3HwFn fn, fn_mask;
  int lds_bytes;
  int waves, rpw;
  void (*wrw)(const __bf16*, const __bf16*, float*, int, int, int, int, int);
  int wrw_lds_bytes, wrw_rows;
  void (*colsum)(const __bf16*, int64_t, float*);
};

template <int C, int COUT, int WAVES, int RPW, int WRW_R>
Conv3HwLaunch make_conv3_hw() {
  using G = Conv3Geom<C, COUT>;
  Conv3HwLaunch l{};
  l.C = C; l.COUT = COUT;
  l.fn = conv3x3p1_fwd_hw_kernel<C, COUT, WAVES, RPW, false>;
  l.fn_mask = conv3x3p1_fwd_hw_kernel<C, COUT, WAVES, RPW, true>;
  l.lds_bytes = G::LDS_BYTES;
  l.waves = WAVES;
  l.rpw = RPW;
  if constexpr (WRW_R > 0) {
    l.wrw = conv3x3p1_wrw_hw_kernel<C, COUT, WRW_R>;
    l.wrw_lds_bytes = Conv3Wrw<C, COUT, WRW_R>::LDS_BYTES;
    l.wrw_rows = 32 * WRW_R;
    l.colsum = colsum_bf16_kernel<COUT>;
  }
  return l;
}

// tile shapes: kConv3Launches' values for the larger geometry of each
// (C, COUT) pair; not swept at other frame sizes
// (profiles/r10_resconv_any_hw.md)
static const Conv3HwLaunch kConv3HwLaunches[] = {
    make_conv3_hw<16, 16, 8, 32, 1>(),
    make_conv3_hw<16, 32, 8, 32, 4>(),
    make_conv3_hw<32, 32, 8, 32, 2>(),
    // input gradient of a 16 -> 32 conv (forward kernels only)
    make_conv3_hw<32, 16, 8, 32, 0>(),
};

const Conv3HwLaunch* find_conv3_hw(int64_t H, int64_t W, int64_t C,
                                   int64_t COUT) {
  if (H < 1 || W < 1) return nullptr;
  for (const auto& l : kConv3HwLaunches)
    if (l.C == C && l.COUT == COUT) return &l;
  return nullptr;
}

// ===========================================================================
// Stem conv of the torso (K2d): 3x3 stride-1 pad-1 at 84x84, C=4 -> 16, the
// one conv the kernels above cannot take (K = 36; an 8-element piece would
// straddle two taps). One pixel's 4 channels are one 8-byte piece, so here
// a TAP is a piece.
//   * padded K layout [kh 0..3][kw 0..3][c 0..3] = 64 columns = two
//     16x16x32 chunks (the second option of the two: no new builtin, the
//     fragment maps are the ones mfma_probe already checks). Slot kw = 3 of
//     every row and the whole row kh = 3 are pad: zeros in LDS and zeros in
//     the im2col fragment. Lane group g = l>>4 of chunk kc holds the taps
//     (kh = 2kc + (g>>1), kw = 2(g&1)) and (kh, kw + 1).
//   * weights staged once per block as [cout][96]: 64 columns + 32 pad, a
//     192-byte row stride — the kPad rule ((row bytes) % 256 in {64, 192});
//     the bare 128-byte row would put lanes l and l+2 on the same banks.
//     The two weight fragments are read from LDS once per wave and kept.
//   * a piece is live iff its tap is inside the image, its slot is no pad
//     and its row is below M; a dead piece is exact zeros and its load sits
//     under the predicate. All live pieces of the wave's rows are issued
//     before the first MFMA.
//   * operands swapped as in conv3x3p1_fwd_kernel (weights as A): a lane
//     holds 4 consecutive couts of one pixel -> one 8-byte store; the 64
//     lanes of a 16-pixel fragment write 512 contiguous bytes.
//   * no flags: the section-entry conv has no relu_in, relu_out or
//     residual. Epilogue in f32: + bias, one rounding to bf16.
// ===========================================================================

using s16x4 = __attribute__((ext_vector_type(4))) short;

struct StemGeom {
  static constexpr int C = 4, COUT = 16;
  static constexpr int K = 9 * C;     // 36, dense (kh, kw, c)
  static constexpr int KP = 64;       // padded [kh 4][kw 4][c 4]
  static constexpr int KCHUNKS = KP / 32;
  static constexpr int LDS_ROW = KP + 32;
  static constexpr int LDS_ELEMS = COUT * LDS_ROW;
  static constexpr int LDS_BYTES = (LDS_ELEMS + COUT) * 2;  // weights + bias
  static_assert((LDS_ROW * 2) % 256 == 64 || (LDS_ROW * 2) % 256 == 192,
                "LDS row stride breaks the bank-spread rule");
  static_assert(LDS_ROW % 8 == 0, "LDS rows must stay 16-byte aligned");
};

template <class HW, int WAVES, int RPW>
__device__ __forceinline__ void conv3x3c4_fwd_body(
    const HW hw,
    const __bf16* __restrict__ in,      // (N,H,W,4) NHWC
    const __bf16* __restrict__ weight,  // (16, 36) = (cout, kh, kw, c)
    const __bf16* __restrict__ bias,    // (16), may be null
    __bf16* __restrict__ out,           // (N,H,W,16)
    int batch) {
  using G = StemGeom;
  constexpr int C = G::C, COUT = G::COUT;
  const int H = hw.H, W = hw.W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* wlds = reinterpret_cast<__bf16*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // ---- stage weights into LDS: [cout][kh 4][kw 4][c], pad slots zero ----
  for (int s = tid; s < COUT * 16; s += WAVES * 64) {
    const int co = s >> 4;
    const int slot = s & 15;
    const int kh = slot >> 2, kw = slot & 3;
    s16x4 v = {};
    if (kh < 3 && kw < 3)
      v = *reinterpret_cast<const s16x4*>(weight + co * G::K +
                                          (kh * 3 + kw) * C);
    *reinterpret_cast<s16x4*>(wlds + co * G::LDS_ROW + slot * C) = v;
  }
  __bf16* blds = wlds + G::LDS_ELEMS;
  if (tid < COUT) blds[tid] = bias ? bias[tid] : (__bf16)0.0f;
  __syncthreads();

  const int M = batch * H * W;
  const int row0 = (blockIdx.x * WAVES + wave) * RPW;
  if (row0 >= M) return;
  constexpr int RFRAG = RPW / 16;
  const int g = lane >> 4;

  // ---- every live piece of the wave's rows goes in flight first ----
  s16x4 a[G::KCHUNKS][RFRAG][2];
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    const int arow = row0 + rf * 16 + (lane & 15);
    const bool row_ok = arow < M;
    const int arc = row_ok ? arow : M - 1;  // ragged tail: decode a real row
    const int rem = arc % (H * W);
    const int p = rem / W;
    const int q = rem - p * W;
    const __bf16* xrow = in + (int64_t)arc * C;  // ((n*H + p)*W + q)*C
#pragma unroll
    for (int kc = 0; kc < G::KCHUNKS; ++kc) {
      const int kh = 2 * kc + (g >> 1);
      const int dy = kh - 1;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int kw = 2 * (g & 1) + h;
        const int dx = kw - 1;
        a[kc][rf][h] = s16x4{};
        const bool live = row_ok && kh < 3 && kw < 3 &&
                          (unsigned)(p + dy) < (unsigned)H &&
                          (unsigned)(q + dx) < (unsigned)W;
        if (live)
          a[kc][rf][h] = *reinterpret_cast<const s16x4*>(
              xrow + (int64_t)(dy * W + dx) * C);
      }
    }
  }

  // the two weight fragments, once per wave
  bf16x8 wa[G::KCHUNKS];
#pragma unroll
  for (int kc = 0; kc < G::KCHUNKS; ++kc)
    wa[kc] = *reinterpret_cast<const bf16x8*>(
        wlds + (lane & 15) * G::LDS_ROW + kc * 32 + g * 8);
  const bf16x4 bv = *reinterpret_cast<const bf16x4*>(blds + g * 4);

  // ---- MFMAs + epilogue: acc[r] = out[row0 + rf*16 + (l&15)][g*4 + r]
#pragma unroll
  for (int rf = 0; rf < RFRAG; ++rf) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < G::KCHUNKS; ++kc) {
      const s16x8 s = __builtin_shufflevector(a[kc][rf][0], a[kc][rf][1], 0, 1,
                                              2, 3, 4, 5, 6, 7);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          wa[kc], __builtin_bit_cast(bf16x8, s), acc, 0, 0, 0);
    }
    const int orow = row0 + rf * 16 + (lane & 15);
    if (orow >= M) continue;
    bf16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = (__bf16)(acc[r] + (float)bv[r]);
    *reinterpret_cast<bf16x4*>(out + (int64_t)orow * COUT + g * 4) = ov;
  }
}

template <int H, int W, int WAVES, int RPW>
__global__ __launch_bounds__(WAVES * 64) void conv3x3c4_fwd_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ weight,
    const __bf16* __restrict__ bias, __bf16* __restrict__ out, int batch) {
  conv3x3c4_fwd_body<HwConst<H, W>, WAVES, RPW>(HwConst<H, W>{}, in, weight,
                                                bias, out, batch);
}

template <int WAVES, int RPW>
__global__ __launch_bounds__(WAVES * 64) void conv3x3c4_fwd_hw_kernel(
    const __bf16* __restrict__ in, const __bf16* __restrict__ weight,
    const __bf16* __restrict__ bias, __bf16* __restrict__ out, int batch,
    int H, int W) {
  conv3x3c4_fwd_body<HwArgs, WAVES, RPW>(HwArgs{H, W}, in, weight, bias, out,
                                         batch);
}

// ---------------------------------------------------------------------------
// Weight gradient of the stem conv, conv3x3p1_wrw_kernel's method:
//   gw[co][(kh,kw,c)] = sum_m gout[m][co] * im2col(x)[m][(kh,kw,c)]
// 32-sample chunks staged plain row-major in LDS, tr_frag fragments, fp32
// MFMA accumulate over the block's m-slice, one fp32 plane per m-slice
// folded in a fixed order by wrw_reduce_kernel (no float atomics).
//   * the staged x tile is [32][kh 3][kw 4][c 4] = 48 columns (+8 pad): one
//     16-column block per kh, whose slot kw = 3 is a zero column. Wave
//     w < 3 owns column block kh = w; wave 3 only stages.
//   * the plane is written DENSE as (16, 36): lane column r < 12 of block
//     kh goes to k = kh*12 + r, so n_elem = 576 = 9*64 and the fold and its
//     bf16 store are the ones every other wrw uses.
//   * a piece (= tap) is live iff its tap is inside the image and its row
//     is below M; dead pieces stay zeros, their address is never formed
//     into a load.
//   * R consecutive chunks per pass; the next pass's pieces are loaded into
//     registers before the current pass's MFMAs.
// Staging: thread t stages rows (t>>3) + 32s, slots (t&7) and (t&7) + 8.
// ---------------------------------------------------------------------------
template <int R>
struct StemWrw {
  static constexpr int C = 4, COUT = 16;
  static constexpr int K = 36;
  static constexpr int SLOTS = 12;                // (kh, kw 0..3) per row
  static constexpr int XIT = 2;                   // slots sj, sj + 8
  static constexpr int XSTRIDE = SLOTS * C + kPadM;  // 56
  static constexpr int GSTRIDE = COUT + kPadM;       // 24
  static constexpr int GP = COUT / 8;             // gout pieces per row
  static constexpr int ROWS = 32 * R;
  static constexpr int GIT = (ROWS * GP + 255) / 256;
  static constexpr int LDS_BYTES = ROWS * (XSTRIDE + GSTRIDE) * 2;
  static_assert(XSTRIDE % 4 == 0 && GSTRIDE % 8 == 0, "aligned LDS rows");
  static_assert(LDS_BYTES <= 64 * 1024, "dynamic LDS limit");
};

template <class HW, int R>
__device__ __forceinline__ void conv3x3c4_wrw_body(
    const HW hw,
    const __bf16* __restrict__ x,     // (N,H,W,4) NHWC
    const __bf16* __restrict__ gout,  // (M, 16) = NHWC grad
    float* __restrict__ gw_part,      // (mblocks, 576 + kPlanePad) fp32
    int batch, int mblocks) {
  using G = StemWrw<R>;
  constexpr int C = G::C, COUT = G::COUT;
  const int H = hw.H, W = hw.W;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* x_t = reinterpret_cast<__bf16*>(smem);  // [ROWS][XSTRIDE]
  __bf16* g_t = x_t + G::ROWS * G::XSTRIDE;       // [ROWS][GSTRIDE]

  const int mb = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  // wave-uniform in an SGPR: the column-block guard below must stay a
  // scalar branch (tr16 reads need the whole wave active)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = batch * H * W;
  const int n_pass = (M + G::ROWS - 1) / G::ROWS;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};

  const int srow = tid >> 3;  // staged sample row 0..31 (+ 32s)
  const int sj = tid & 7;     // first slot of that row

  s16x4 xr[R][G::XIT];
  s16x8 gr[G::GIT];
  auto load_pass = [&](int mc) __attribute__((always_inline)) {
    const int m0 = mc * G::ROWS;
#pragma unroll
    for (int s = 0; s < R; ++s) {
      const int m = m0 + s * 32 + srow;
      const bool valid = m < M;
      const int mcl = valid ? m : 0;
      const int rem = mcl % (H * W);
      const int p = rem / W;
      const int q = rem - p * W;
      const __bf16* xrow = x + (int64_t)mcl * C;  // ((n*H + p)*W + q)*C
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        xr[s][i] = s16x4{};
        const int slot = sj + 8 * i;
        const int kh = slot >> 2, kw = slot & 3;
        const int dy = kh - 1, dx = kw - 1;
        const bool live = valid && slot < G::SLOTS && kw < 3 &&
                          (unsigned)(p + dy) < (unsigned)H &&
                          (unsigned)(q + dx) < (unsigned)W;
        if (live)
          xr[s][i] = *reinterpret_cast<const s16x4*>(
              xrow + (int64_t)(dy * W + dx) * C);
      }
    }
#pragma unroll
    for (int t = 0; t < G::GIT; ++t) {
      const int piece = tid + 256 * t;
      const int m = m0 + piece / G::GP;
      gr[t] = s16x8{};
      if (piece < G::ROWS * G::GP && m < M)
        gr[t] = *reinterpret_cast<const s16x8*>(
            gout + (int64_t)m * COUT + (piece % G::GP) * 8);
    }
  };

  if (mb < n_pass) load_pass(mb);
  for (int mc = mb; mc < n_pass; mc += mblocks) {
    // ---- registers -> LDS (pad slots get their zeros here)
#pragma unroll
    for (int s = 0; s < R; ++s)
#pragma unroll
      for (int i = 0; i < G::XIT; ++i) {
        const int slot = sj + 8 * i;
        if (slot < G::SLOTS)
          *reinterpret_cast<s16x4*>(x_t + (s * 32 + srow) * G::XSTRIDE +
                                    slot * C) = xr[s][i];
      }
#pragma unroll
    for (int t = 0; t < G::GIT; ++t) {
      const int piece = tid + 256 * t;
      if (piece < G::ROWS * G::GP)
        *reinterpret_cast<s16x8*>(g_t + (piece / G::GP) * G::GSTRIDE +
                                  (piece % G::GP) * 8) = gr[t];
    }
    __syncthreads();
    if (mc + mblocks < n_pass) load_pass(mc + mblocks);
    // ---- fragments via tr16 reads + MFMA: wave kh against the cout block
    if (wave < 3) {
#pragma unroll
      for (int s = 0; s < R; ++s) {
        const bf16x8 gf = tr_frag<G::GSTRIDE>(g_t + s * 32 * G::GSTRIDE, lane, 0);
        const bf16x8 xf =
            tr_frag<G::XSTRIDE>(x_t + s * 32 * G::XSTRIDE, lane, wave);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gf, xf, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // ---- epilogue: this m-slice's partial, dense (16, 36), to its own plane
  float* plane = gw_part + (int64_t)mb * (COUT * G::K + kPlanePad);
  const int col = lane & 15;
  if (wave < 3 && col < 12) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int cout = (lane >> 4) * 4 + r;
      plane[cout * G::K + wave * 12 + col] = acc[r];
    }
  }
}

template <int H, int W, int R>
__global__ __launch_bounds__(256) void conv3x3c4_wrw_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ gout,
    float* __restrict__ gw_part, int batch, int mblocks) {
  conv3x3c4_wrw_body<HwConst<H, W>, R>(HwConst<H, W>{}, x, gout, gw_part,
                                       batch, mblocks);
}

template <int R>
__global__ __launch_bounds__(256) void conv3x3c4_wrw_hw_kernel(
    const __bf16* __restrict__ x, const __bf16* __restrict__ gout,
    float* __restrict__ gw_part, int batch, int mblocks, int H, int W) {
  conv3x3c4_wrw_body<HwArgs, R>(HwArgs{H, W}, x, gout, gw_part, batch,
                                mblocks);
}

// the stem's own one-entry table (it does not go through kConv3Launches)
struct StemLaunch {
  int H, W, C, COUT;
  void (*fwd)(const __bf16*, const __bf16*, const __bf16*, __bf16*, int);
  int lds_bytes, waves, rpw;
  void (*wrw)(const __bf16*, const __bf16*, float*, int, int);
  int wrw_lds_bytes, wrw_rows;
  void (*colsum)(const __bf16*, int64_t, float*);
};

template <int H, int W, int WAVES, int RPW, int WRW_R>
StemLaunch make_stem() {
  StemLaunch l{};
  l.H = H; l.W = W; l.C = StemGeom::C; l.COUT = StemGeom::COUT;
  l.fwd = conv3x3c4_fwd_kernel<H, W, WAVES, RPW>;
  l.lds_bytes = StemGeom::LDS_BYTES;
  l.waves = WAVES;
  l.rpw = RPW;
  l.wrw = conv3x3c4_wrw_kernel<H, W, WRW_R>;
  l.wrw_lds_bytes = StemWrw<WRW_R>::LDS_BYTES;
  l.wrw_rows = 32 * WRW_R;
  l.colsum = colsum_bf16_kernel<StemGeom::COUT>;
  return l;
}

static const StemLaunch kStemLaunches[] = {
    // cfg/impala_resnet.json's first conv. 8 waves x 32 rows and WRW_R = 1
    // are what the A/B and the trace of profiles/r08_stem_conv.md ran; its
    // sweep has 4x64 at 0.91x the forward's time and WRW_R = 4 / 8 at
    // 0.92x / 0.89x the weight gradient's, left for the change of default
    make_stem<84, 84, 8, 32, 1>(),
};

const StemLaunch* find_stem(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  for (const auto& l : kStemLaunches)
    if (l.H == H && l.W == W && l.C == C && l.COUT == COUT) return &l;
  return nullptr;
}

// the stem's run-time entry (the _hw bindings): StemLaunch's fields, H and
// W as two trailing kernel arguments
struct StemHwLaunch {
  int C, COUT;
  void (*fwd)(const __bf16*, const __bf16*, const __bf16*, __bf16*, int, int,
              int);
  int lds_bytes, waves, rpw;
  void (*wrw)(const __bf16*, const __bf16*, float*, int, int, int, int);
  int wrw_lds_bytes, wrw_rows;
  void (*colsum)(const __bf16*, int64_t, float*);
};

template <int WAVES, int RPW, int WRW_R>
StemHwLaunch make_stem_hw() {
  StemHwLaunch l{};
  l.C = StemGeom::C; l.COUT = StemGeom::COUT;
  l.fwd = conv3x3c4_fwd_hw_kernel<WAVES, RPW>;
  l.lds_bytes = StemGeom::LDS_BYTES;
  l.waves = WAVES;
  l.rpw = RPW;
  l.wrw = conv3x3c4_wrw_hw_kernel<WRW_R>;
  l.wrw_lds_bytes = StemWrw<WRW_R>::LDS_BYTES;
  l.wrw_rows = 32 * WRW_R;
  l.colsum = colsum_bf16_kernel<StemGeom::COUT>;
  return l;
}

static const StemHwLaunch kStemHwLaunches[] = {
    make_stem_hw<8, 32, 1>(),  // the table entry's tile shapes
};

const StemHwLaunch* find_stem_hw(int64_t C, int64_t COUT) {
  for (const auto& l : kStemHwLaunches)
    if (l.C == C && l.COUT == COUT) return &l;
  return nullptr;
}

// ===========================================================================
// Max-pool 3x3 stride 2 pad 1 (dilation 1, floor mode) of the torso, NHWC
// bf16, forward and backward. H, W and C are run-time values, C % 16 == 0;
// P = (H-1)/2 + 1, Q = (W-1)/2 + 1. Both kernels stream: one lane owns 16
// channels of one pixel (two 16-byte pieces), lanes run along (n, row, col,
// channel group), so a wave reads and writes contiguous memory.
//
//   * forward: lane = output pixel. Taps are scanned in (kh, kw) order; the
//     first in-bounds tap initialises maximum and index, a later one
//     replaces them iff v > m || isnan(v) (the library's rule: ties keep
//     the earliest tap, +0/-0 do not replace each other, NaN propagates and
//     the last NaN takes the index). Written here as m = -inf, index =
//     first in-bounds tap, then the rule over every in-bounds tap: the first
//     either replaces (v > -inf or NaN) or is -inf itself. The winner's
//     bf16 bits are stored as they are. An out-of-bounds tap is never
//     loaded. The index plane is uint8, same shape and layout as out,
//     holding kh*3 + kw; WITH_IDX=false drops it (no gradient wanted).
//   * backward: a gather, lane = INPUT pixel (h, w). Row h lies in window
//     po = h/2 at kh = 1 (h even), or in po = (h-1)/2 at kh = 2 and
//     po = (h+1)/2 (if < P) at kh = 0 (h odd); columns alike: 1, 2 or 4
//     windows. gx = sum of gout[po,qo] where idx[po,qo] names this pixel's
//     tap, in ascending (po, qo) order, in f32, rounded to bf16 once. Every
//     gx element is written exactly once: no zero fill, no atomics, and the
//     result does not depend on scheduling.
// ===========================================================================

using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

template <bool WITH_IDX>
__global__ __launch_bounds__(256) void maxpool3x3s2_fwd_kernel(
    const __bf16* __restrict__ x,  // (N,H,W,C)
    __bf16* __restrict__ out,      // (N,P,Q,C)
    uint8_t* __restrict__ idx,     // (N,P,Q,C), WITH_IDX only
    int lanes,                     // N*P*Q*CG
    int H, int W, int P, int Q, int CG) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)lanes) return;
  const unsigned pix = i / (unsigned)CG;  // (n*P + p)*Q + q
  const unsigned cg = i - pix * (unsigned)CG;
  const unsigned np = pix / (unsigned)Q;
  const int q = (int)(pix - np * (unsigned)Q);
  const unsigned n = np / (unsigned)P;
  const int p = (int)(np - n * (unsigned)P);
  const int C = CG * 16;
  const int h0 = 2 * p - 1, w0 = 2 * q - 1;
  const __bf16* xin = x + (int64_t)n * H * W * C + cg * 16;

  float m[16];
  unsigned ix[16];
  const unsigned first = (p == 0 ? 3u : 0u) + (q == 0 ? 1u : 0u);
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    m[c] = -__builtin_inff();
    ix[c] = first;
  }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int h = h0 + kh;
    // a row's three taps go in flight together
    u32x4 v[3][2] = {};
    bool live[3];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int w = w0 + kw;
      live[kw] = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
      if (live[kw]) {
        const u32x4* s =
            reinterpret_cast<const u32x4*>(xin + ((int64_t)h * W + w) * C);
        v[kw][0] = s[0];
        v[kw][1] = s[1];
      }
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      if (!live[kw]) continue;
      const unsigned tap = kh * 3 + kw;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        // bf16 -> f32 is the bits moved up: compare in f32, keep the bits
        const unsigned word = v[kw][c >> 3][(c >> 1) & 3];
        const float f = __builtin_bit_cast(
            float, (c & 1) ? (word & 0xffff0000u) : (word << 16));
        const bool take = f > m[c] || f != f;
        m[c] = take ? f : m[c];
        ix[c] = take ? tap : ix[c];
      }
    }
  }

  const int64_t o = (int64_t)pix * C + cg * 16;
  u32x4 ov[2];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    ov[j >> 2][j & 3] = (__builtin_bit_cast(unsigned, m[2 * j]) >> 16) |
                        (__builtin_bit_cast(unsigned, m[2 * j + 1]) &
                         0xffff0000u);
  u32x4* od = reinterpret_cast<u32x4*>(out + o);
  od[0] = ov[0];
  od[1] = ov[1];
  if constexpr (WITH_IDX) {
    u32x4 iv;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      iv[j] = ix[4 * j] | (ix[4 * j + 1] << 8) | (ix[4 * j + 2] << 16) |
              (ix[4 * j + 3] << 24);
    *reinterpret_cast<u32x4*>(idx + o) = iv;
  }
}

__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(
    const __bf16* __restrict__ gout,  // (N,P,Q,C)
    const uint8_t* __restrict__ idx,  // (N,P,Q,C)
    __bf16* __restrict__ gx,          // (N,H,W,C)
    int lanes,                        // N*H*W*CG
    int H, int W, int P, int Q, int CG) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)lanes) return;
  const unsigned pix = i / (unsigned)CG;  // (n*H + h)*W + w
  const unsigned cg = i - pix * (unsigned)CG;
  const unsigned nh = pix / (unsigned)W;
  const int w = (int)(pix - nh * (unsigned)W);
  const unsigned n = nh / (unsigned)H;
  const int h = (int)(nh - n * (unsigned)H);
  const int C = CG * 16;
  const int64_t img = (int64_t)n * P * Q * C + cg * 16;

  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int po = (h >> 1) + a;
    const int kh = h + 1 - 2 * po;  // 1 | 2 then 0
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int qo = (w >> 1) + b;
      const int kw = w + 1 - 2 * qo;
      // the second window exists for odd coordinates only, and not past
      // the last one
      const bool live = (a == 0 || ((h & 1) && po < P)) &&
                        (b == 0 || ((w & 1) && qo < Q));
      if (!live) continue;
      const int64_t o = img + ((int64_t)po * Q + qo) * C;
      const u32x4 iv = *reinterpret_cast<const u32x4*>(idx + o);
      const u32x4* gs = reinterpret_cast<const u32x4*>(gout + o);
      const u32x4 g0 = gs[0], g1 = gs[1];
      const unsigned tap = (unsigned)(kh * 3 + kw);
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const unsigned word = (c < 8 ? g0 : g1)[(c >> 1) & 3];
        const float g = __builtin_bit_cast(
            float, (c & 1) ? (word & 0xffff0000u) : (word << 16));
        const unsigned t = (iv[c >> 2] >> (8 * (c & 3))) & 0xffu;
        acc[c] += t == tap ? g : 0.f;
      }
    }
  }

  u32x4 ov[2];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned lo =
        __builtin_bit_cast(unsigned short, (__bf16)acc[2 * j]);
    const unsigned hi =
        __builtin_bit_cast(unsigned short, (__bf16)acc[2 * j + 1]);
    ov[j >> 2][j & 3] = lo | (hi << 16);
  }
  u32x4* od = reinterpret_cast<u32x4*>(gx + (int64_t)pix * C + cg * 16);
  od[0] = ov[0];
  od[1] = ov[1];
}

// ===========================================================================
// Geometry table of the strided no-pad convs: ONE entry per
// (H, W, C, KH, KW, S, COUT, u8) carries every kernel of that geometry, so
// a new geometry or variant is one line here.
// ===========================================================================

// run-time twin of ConvGeom's template arguments
struct Geom {
  int64_t H, W, C, KH, KW, S, COUT;
  bool u8;
  int64_t P() const { return (H - KH) / S + 1; }
  int64_t Q() const { return (W - KW) / S + 1; }
  int64_t K() const { return KH * KW * C; }
  bool operator==(const Geom& o) const {
    return H == o.H && W == o.W && C == o.C && KH == o.KH && KW == o.KW &&
           S == o.S && COUT == o.COUT && u8 == o.u8;
  }
};

// the one matcher of every table whose entries start with a Geom g
template <typename Entry, size_t N>
const Entry* find_geom(const Entry (&table)[N], const Geom& g) {
  for (const auto& e : table)
    if (e.g == g) return &e;
  return nullptr;
}

using FwdFn = void (*)(const void*, const __bf16*, const __bf16*, __bf16*, int);
using GroupedFn = void (*)(const ConvJobs, int, int);

struct ConvEntry {
  Geom g;
  // forwards; waves/rpw/lds_bytes are shared by all four (the CHW-out
  // variants run the tile shape of their NHWC twins). Null: no such variant.
  int waves, rpw, lds_bytes;
  FwdFn fwd;
  GroupedFn grouped;
  FwdFn fwd_chw;
  GroupedFn grouped_chw;
  // weight-grad + its bias-grad column sum (null in the tuning table)
  void (*wrw)(const void*, const __bf16*, float*, int, int);
  int wrw_lds_bytes, ktiles;
  void (*colsum)(const __bf16*, int64_t, float*);
};

enum : int { kGrouped = 1, kChw = 2, kChwGrouped = 4, kWrw = 8 };

template <int H, int W, int C, int KH, int KW, int S, int COUT, bool U8,
          int WAVES, int RPW, int FLAGS>
ConvEntry make_conv() {
  using G = ConvGeom<H, W, C, KH, KW, S, COUT, U8>;
  // conv_wrw recovers KH/KW from the output extent
  static_assert((H - KH) % S == 0 && (W - KW) % S == 0, "ragged last window");
  ConvEntry e{};
  e.g = Geom{H, W, C, KH, KW, S, COUT, U8};
  e.waves = WAVES;
  e.rpw = RPW;
  e.lds_bytes = (int)(G::LDS_ELEMS * sizeof(__bf16));
  e.fwd = conv_fwd_kernel<H, W, C, KH, KW, S, COUT, U8, WAVES, RPW, false>;
  if constexpr (FLAGS & kGrouped)
    e.grouped =
        conv_fwd_grouped_kernel<H, W, C, KH, KW, S, COUT, U8, WAVES, RPW, false>;
  if constexpr (FLAGS & kChw)
    e.fwd_chw = conv_fwd_kernel<H, W, C, KH, KW, S, COUT, U8, WAVES, RPW, true>;
  if constexpr (FLAGS & kChwGrouped)
    e.grouped_chw =
        conv_fwd_grouped_kernel<H, W, C, KH, KW, S, COUT, U8, WAVES, RPW, true>;
  if constexpr (FLAGS & kWrw) {
    static_assert(G::K % 64 == 0, "wrw needs K % 64 == 0");
    e.wrw = conv_wrw_kernel<H, W, C, KH, KW, S, COUT, U8>;
    e.wrw_lds_bytes = (int)(32 * (64 + kPadM + COUT + kPadM) * sizeof(__bf16));
    e.ktiles = G::K / 64;
    e.colsum = colsum_bf16_kernel<COUT>;
  }
  return e;
}

static const ConvEntry kConvs[] = {
    // Ape-X / R2D2 stack (cfg/ape_x.json:38-51); WAVES/RPW picked by the
    // variant sweep in tools/gpu_conv_tune.py (profiles/). The last conv of a
    // stack also has the CHW-out (flatten-fusing) forwards.
    make_conv<84, 84, 4, 8, 8, 4, 32, true, 8, 32, kGrouped | kWrw>(),
    make_conv<84, 84, 4, 8, 8, 4, 32, false, 8, 32, kGrouped | kWrw>(),
    make_conv<20, 20, 32, 4, 4, 2, 64, false, 8, 16, kGrouped | kWrw>(),
    make_conv<9, 9, 64, 3, 3, 1, 64, false, 8, 16,
              kGrouped | kChw | kChwGrouped | kWrw>(),
    // IMPALA stack (cfg/impala.json:26-39)
    make_conv<84, 84, 4, 8, 8, 4, 16, true, 8, 16, kWrw>(),
    make_conv<84, 84, 4, 8, 8, 4, 16, false, 8, 16, kWrw>(),
    make_conv<20, 20, 16, 4, 4, 2, 32, false, 8, 16, kChw | kWrw>(),
};

// variant table for on-GPU tuning (tools/gpu_conv_tune.py): single-job NHWC
// forward only
static const ConvEntry kVariants[] = {
    make_conv<84, 84, 4, 8, 8, 4, 32, true, 4, 16, 0>(),
    make_conv<84, 84, 4, 8, 8, 4, 32, true, 8, 16, 0>(),
    make_conv<84, 84, 4, 8, 8, 4, 32, true, 4, 32, 0>(),
    make_conv<84, 84, 4, 8, 8, 4, 32, true, 8, 32, 0>(),
    make_conv<20, 20, 32, 4, 4, 2, 64, false, 4, 16, 0>(),
    make_conv<20, 20, 32, 4, 4, 2, 64, false, 8, 16, 0>(),
    make_conv<20, 20, 32, 4, 4, 2, 64, false, 4, 32, 0>(),
    make_conv<20, 20, 32, 4, 4, 2, 64, false, 8, 32, 0>(),
    make_conv<9, 9, 64, 3, 3, 1, 64, false, 4, 16, 0>(),
    make_conv<9, 9, 64, 3, 3, 1, 64, false, 8, 16, 0>(),
    make_conv<9, 9, 64, 3, 3, 1, 64, false, 4, 32, 0>(),
    make_conv<9, 9, 64, 3, 3, 1, 64, false, 8, 32, 0>(),
};

struct DgradEntry {
  Geom g;  // u8 is always false: dgrad never meets the u8 first layer
  void (*fn)(const __bf16*, const __bf16*, __bf16*, int);
  int waves, rpw;
};

template <int H, int W, int C, int KH, int KW, int S, int COUT, int WAVES = 8,
          int RPW = 16>
DgradEntry make_dgrad() {
  return DgradEntry{Geom{H, W, C, KH, KW, S, COUT, false},
                    conv_dgrad_kernel<H, W, C, KH, KW, S, COUT, WAVES, RPW>,
                    WAVES, RPW};
}

static const DgradEntry kDgrad[] = {
    make_dgrad<20, 20, 32, 4, 4, 2, 64>(),  // apex/r2d2 conv2
    make_dgrad<9, 9, 64, 3, 3, 1, 64>(),    // apex/r2d2 conv3
    make_dgrad<20, 20, 16, 4, 4, 2, 32>(),  // impala conv2
};

const ConvEntry* find_conv(int64_t H, int64_t W, int64_t C, int64_t KH,
                           int64_t KW, int64_t S, int64_t COUT, bool u8) {
  return find_geom(kConvs, Geom{H, W, C, KH, KW, S, COUT, u8});
}

// ===========================================================================
// Argument checks. Every tensor a kernel dereferences goes through one of
// these before its pointer is taken: on the device, the expected dtype, and
// exactly the sizes and memory layout the geometry implies — an
// out-of-bounds launch takes the card down, not just the test.
// ===========================================================================

constexpr auto kBF16 = torch::kBFloat16;

hipStream_t cur_stream() {
  return (hipStream_t)at::cuda::getCurrentCUDAStream().stream();
}

void check_dev(const torch::Tensor& t, at::ScalarType dtype, const char* what) {
  TORCH_CHECK(t.defined() && t.is_cuda(), what, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == dtype, what, " must be ", dtype, ", got ",
              t.scalar_type());
}

// plain contiguous tensor of exactly `sizes`
void check_rows(const torch::Tensor& t, at::ScalarType dtype,
                at::IntArrayRef sizes, const char* what) {
  check_dev(t, dtype, what);
  TORCH_CHECK(t.sizes() == sizes && t.is_contiguous(), what,
              " must be contiguous ", sizes, ", got ", t.sizes());
}

// logical (n, c, h, w) tensor in channels_last (NHWC) memory
void check_nhwc(const torch::Tensor& t, at::ScalarType dtype, int64_t n,
                int64_t c, int64_t h, int64_t w, const char* what) {
  check_dev(t, dtype, what);
  TORCH_CHECK(t.sizes() == at::IntArrayRef({n, c, h, w}), what, " must be (",
              n, ", ", c, ", ", h, ", ", w, "), got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), what,
              " must be channels_last");
}

// optional (n) bf16 vector: undefined or empty means "none"
const __bf16* opt_vec(const torch::Tensor& t, int64_t n, const char* what) {
  if (!t.defined() || t.numel() == 0) return nullptr;
  check_rows(t, kBF16, {n}, what);
  return (const __bf16*)t.data_ptr();
}

// kernels index rows with int
int checked_rows(int64_t rows, const char* what) {
  TORCH_CHECK(rows < (int64_t)1 << 31, what, ": too many rows");
  return (int)rows;
}

// geometry of a forward call, from its first job
Geom geom_of(const torch::Tensor& in, const torch::Tensor& weight,
             int64_t stride) {
  TORCH_CHECK(in.dim() == 4 && weight.dim() == 4 && stride >= 1,
              "conv wants 4-D input and weight and a positive stride");
  return Geom{in.size(2), in.size(3), in.size(1), weight.size(2),
              weight.size(3), stride, weight.size(0),
              in.scalar_type() == torch::kUInt8};
}

// The one forward launch path: checks every job against entry e, then runs
// e's single-job kernel for one job (grid = row tiles) and its grouped kernel
// for 2..kMaxConvJobs (grid = tiles * njobs). biases is empty (no job has a
// bias) or one tensor per job.
void launch_conv_fwd(const ConvEntry& e, const std::vector<torch::Tensor>& ins,
                     const std::vector<torch::Tensor>& weights,
                     const std::vector<torch::Tensor>& biases,
                     const std::vector<torch::Tensor>& outs, bool chw_out) {
  const Geom& g = e.g;
  const int njobs = (int)ins.size();
  const FwdFn single = chw_out ? e.fwd_chw : e.fwd;
  const GroupedFn grouped = chw_out ? e.grouped_chw : e.grouped;
  TORCH_CHECK(njobs > 1 ? grouped != nullptr : single != nullptr, "no ",
              njobs > 1 ? "grouped" : "fused",
              " conv kernel for this geometry: ", g.H, "x", g.W, "x", g.C,
              " k", g.KH, "x", g.KW, " s", g.S, " -> ", g.COUT, " u8=", g.u8,
              " chw=", chw_out);
  const int64_t N = ins[0].size(0), P = g.P(), Q = g.Q();
  const int M = checked_rows(N * P * Q, "conv_fwd");
  ConvJobs jobs{};
  for (int j = 0; j < njobs; ++j) {
    check_nhwc(ins[j], g.u8 ? torch::kUInt8 : kBF16, N, g.C, g.H, g.W,
               "conv input (jobs share N and geometry)");
    check_nhwc(weights[j], kBF16, g.COUT, g.C, g.KH, g.KW, "conv weight");
    if (chw_out)
      check_rows(outs[j], kBF16, {N, g.COUT * P * Q}, "conv CHW output");
    else
      check_nhwc(outs[j], kBF16, N, g.COUT, P, Q, "conv output");
    jobs.in[j] = ins[j].data_ptr();
    jobs.weight[j] = (const __bf16*)weights[j].data_ptr();
    jobs.out[j] = (__bf16*)outs[j].data_ptr();
    jobs.bias[j] =
        biases.empty() ? nullptr : opt_vec(biases[j], g.COUT, "conv bias");
  }
  if (M == 0) return;
  const int rows_per_block = e.waves * e.rpw;
  const int tiles = (M + rows_per_block - 1) / rows_per_block;
  if (njobs == 1)
    hipLaunchKernelGGL(single, dim3(tiles), dim3(e.waves * 64), e.lds_bytes,
                       cur_stream(), jobs.in[0], jobs.weight[0], jobs.bias[0],
                       jobs.out[0], (int)N);
  else
    hipLaunchKernelGGL(grouped, dim3(tiles * njobs), dim3(e.waves * 64),
                       e.lds_bytes, cur_stream(), jobs, njobs, (int)N);
}

// Blocks of L's weight-grad kernel that the current device holds at once;
// asked of the runtime on the first call per (geometry, device) (a host-side
// query: nothing is enqueued) and kept. Threads that race on an empty slot
// all store the same value. The m-grid, and with it the summation order and
// the last bits of gw, follows this figure: results are reproducible on one
// device model, not across parts with another CU count or occupancy.
constexpr int kMaxDevices = 64;

// per_dev: one table entry's kMaxDevices slots
int resident_blocks(std::atomic<int>* per_dev, const void* fn, int lds_bytes,
                    const char* who) {
  const int dev = at::cuda::current_device();
  TORCH_CHECK(dev >= 0 && dev < kMaxDevices, who, ": device index");
  std::atomic<int>& slot = per_dev[dev];
  int r = slot.load(std::memory_order_relaxed);
  if (r == 0) {
    int per_cu = 0;
    TORCH_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &per_cu, fn, 256, lds_bytes) == hipSuccess && per_cu > 0,
                who, ": occupancy query failed");
    r = per_cu * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    slot.store(r, std::memory_order_relaxed);
  }
  return r;
}

int wrw_resident_blocks(const Conv3Launch& L) {
  static std::atomic<int> cache[std::size(kConv3Launches)][kMaxDevices] = {};
  return resident_blocks(cache[&L - kConv3Launches], (const void*)L.wrw,
                         L.wrw_lds_bytes, "conv3x3p1_wrw");
}

int wrw_resident_blocks(const StemLaunch& L) {
  static std::atomic<int> cache[std::size(kStemLaunches)][kMaxDevices] = {};
  return resident_blocks(cache[&L - kStemLaunches], (const void*)L.wrw,
                         L.wrw_lds_bytes, "conv3x3c4_wrw");
}

// the run-time kernels have their own figures: their register counts are
// not the table kernels'
int wrw_resident_blocks(const Conv3HwLaunch& L) {
  static std::atomic<int> cache[std::size(kConv3HwLaunches)][kMaxDevices] = {};
  return resident_blocks(cache[&L - kConv3HwLaunches], (const void*)L.wrw,
                         L.wrw_lds_bytes, "conv3x3p1_wrw (run-time H, W)");
}

int wrw_resident_blocks(const StemHwLaunch& L) {
  static std::atomic<int> cache[std::size(kStemHwLaunches)][kMaxDevices] = {};
  return resident_blocks(cache[&L - kStemHwLaunches], (const void*)L.wrw,
                         L.wrw_lds_bytes, "conv3x3c4_wrw_hw");
}

// m-grid of an ordered weight gradient from its pass count, the smallest of
// three: a block should meet at least 8 passes, so the plane it writes (and
// the fold reads back) stays well below the input bytes it streams; all
// planes together stay within 16 MiB; and no more blocks than are resident
// at once (a second, part-filled round of blocks would only add planes)
int wrw_m_grid(int n_pass, int64_t plane_bytes, int resident) {
  int mb = (n_pass + 7) / 8;
  const int mb_cap = (int)(((int64_t)16 << 20) / plane_bytes);
  if (mb > mb_cap) mb = mb_cap;
  if (mb > resident) mb = resident;
  return mb < 1 ? 1 : mb;
}

void launch_wrw_reduce(const torch::Tensor& part, int mb,
                       const torch::Tensor& b_part, int64_t COUT,
                       torch::Tensor& gw_ws, torch::Tensor& gb_ws, bool bias);

// Ordered fold shared by every weight-grad: wrw_reduce_kernel sums the mb
// partial planes of `part` into gw_ws (fp32 workspace, or bf16 = the
// gradient itself); with bias, colsum's per-block column sums of gout
// (M, COUT) fold into gb_ws in the same launch.
void launch_wrw_fold(const torch::Tensor& part, int mb,
                     const torch::Tensor& gout, int M, int64_t COUT,
                     void (*colsum)(const __bf16*, int64_t, float*),
                     torch::Tensor& gw_ws, torch::Tensor& gb_ws, bool bias) {
  torch::Tensor b_part;
  if (bias) {
    b_part = torch::empty({(int64_t)kColsumBlocks, COUT}, part.options());
    hipLaunchKernelGGL(colsum, dim3(kColsumBlocks), dim3(256), 0,
                       cur_stream(), (const __bf16*)gout.data_ptr(),
                       (int64_t)M, b_part.data_ptr<float>());
  }
  launch_wrw_reduce(part, mb, b_part, COUT, gw_ws, gb_ws, bias);
}

// wrw_reduce_kernel on its own: b_part holds kColsumBlocks x COUT column-sum
// partials when bias is set
void launch_wrw_reduce(const torch::Tensor& part, int mb,
                       const torch::Tensor& b_part, int64_t COUT,
                       torch::Tensor& gw_ws, torch::Tensor& gb_ws, bool bias) {
  auto st = cur_stream();
  const int n_elem = (int)gw_ws.numel();
  const bool bf16_out = gw_ws.scalar_type() == kBF16;
  const int e_blocks = (n_elem + 63) / 64;
  const float* b_part_ptr =
      bias ? (const float*)b_part.data_ptr<float>() : nullptr;
  if (bf16_out)
    hipLaunchKernelGGL(wrw_reduce_kernel<__bf16>,
                       dim3(e_blocks + (bias ? 1 : 0)), dim3(256), 0, st,
                       (const float*)part.data_ptr<float>(), mb, n_elem,
                       (__bf16*)gw_ws.data_ptr(), b_part_ptr, kColsumBlocks,
                       (int)COUT, bias ? (__bf16*)gb_ws.data_ptr() : nullptr);
  else
    hipLaunchKernelGGL(wrw_reduce_kernel<float>,
                       dim3(e_blocks + (bias ? 1 : 0)), dim3(256), 0, st,
                       (const float*)part.data_ptr<float>(), mb, n_elem,
                       gw_ws.data_ptr<float>(), b_part_ptr, kColsumBlocks,
                       (int)COUT, bias ? gb_ws.data_ptr<float>() : nullptr);
}

// what each tensor of a launch_conv3 call is named in its error messages
struct Conv3Labels {
  const char *in, *out, *bias, *residual, *mask;
};

// The one launch path of conv3x3p1_fwd_kernel (forward and input gradient):
// in (N,C,H,W) / out (N,COUT,H,W) logical channels_last bf16; w is COUT*9C
// checked bf16 elements in (cout, kh, kw, c) order; residual and mask are
// empty or shaped like out. mask selects the MASK instantiation. With
// flip_from (a checked (COUT', C', 3, 3) weight of the same numel), w is a
// workspace that conv3x3_w_flip_kernel fills first — after every check, so
// a rejected call launches nothing.
void launch_conv3(const torch::Tensor& in, const __bf16* w,
                  const __bf16* flip_from, const torch::Tensor& bias,
                  const torch::Tensor& residual, const torch::Tensor& mask,
                  const torch::Tensor& out, int64_t COUT, bool relu_in,
                  bool relu_out, bool any_hw, const Conv3Labels& lb) {
  const int64_t N = in.size(0), C = in.size(1), H = in.size(2), W = in.size(3);
  check_nhwc(in, kBF16, N, C, H, W, lb.in);
  check_nhwc(out, kBF16, N, COUT, H, W, lb.out);
  TORCH_CHECK(out.data_ptr() != in.data_ptr(), lb.out, " must not alias ",
              lb.in, " (not in-place)");
  // 16-byte pieces of in / weight, 8-byte pieces of out / residual / mask
  TORCH_CHECK((uintptr_t)in.data_ptr() % 16 == 0, lb.in, " is misaligned");
  TORCH_CHECK((uintptr_t)w % 16 == 0, lb.in, "'s weight is misaligned");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 8 == 0, lb.out, " is misaligned");
  // the geometry table first, then the (C, COUT) run-time entry; any_hw
  // (tests and the measurement) skips the table
  const Conv3Launch* L = any_hw ? nullptr : find_conv3(H, W, C, COUT);
  const Conv3HwLaunch* R = L ? nullptr : find_conv3_hw(H, W, C, COUT);
  TORCH_CHECK(L || R, "no 3x3 pad-1 conv kernel for this geometry: ", H, "x",
              W, "x", C, " -> ", COUT);
  const int M = checked_rows(N * H * W, lb.out);
  const __bf16* bias_ptr = opt_vec(bias, COUT, lb.bias);
  // optional tensor shaped like out: undefined or empty means "none"
  auto like_out = [&](const torch::Tensor& t, const char* what) {
    if (!t.defined() || t.numel() == 0) return (const __bf16*)nullptr;
    check_nhwc(t, kBF16, N, COUT, H, W, what);
    TORCH_CHECK((uintptr_t)t.data_ptr() % 8 == 0, what, " is misaligned");
    return (const __bf16*)t.data_ptr();
  };
  const __bf16* res_ptr = like_out(residual, lb.residual);
  const __bf16* mask_ptr = like_out(mask, lb.mask);
  if (N == 0) return;
  if (flip_from) {
    // W'[ci][tap][co]: the flipped weight's (cout', c') = (C, COUT) here
    const int total = (int)(9 * C * COUT);
    hipLaunchKernelGGL(conv3x3_w_flip_kernel, dim3((total + 255) / 256),
                       dim3(256), 0, cur_stream(), flip_from,
                       const_cast<__bf16*>(w), (int)COUT, (int)C);
  }
  const int rows_per_block = L ? L->waves * L->rpw : R->waves * R->rpw;
  const int blocks = (M + rows_per_block - 1) / rows_per_block;
  if (L)
    hipLaunchKernelGGL(mask_ptr ? L->fn_mask : L->fn, dim3(blocks),
                       dim3(L->waves * 64), L->lds_bytes, cur_stream(),
                       (const __bf16*)in.data_ptr(), w, bias_ptr, res_ptr,
                       mask_ptr, (__bf16*)out.data_ptr(), (int)N,
                       relu_in ? 1 : 0, relu_out ? 1 : 0);
  else
    hipLaunchKernelGGL(mask_ptr ? R->fn_mask : R->fn, dim3(blocks),
                       dim3(R->waves * 64), R->lds_bytes, cur_stream(),
                       (const __bf16*)in.data_ptr(), w, bias_ptr, res_ptr,
                       mask_ptr, (__bf16*)out.data_ptr(), (int)N,
                       relu_in ? 1 : 0, relu_out ? 1 : 0, (int)H, (int)W);
}

}  // namespace

// ===========================================================================
// Host entry points
// ===========================================================================

void mfma_probe(torch::Tensor A, torch::Tensor B, torch::Tensor C) {
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)at::cuda::getCurrentCUDAStream().stream(),
                     (const __bf16*)A.data_ptr(), (const __bf16*)B.data_ptr(),
                     C.data_ptr<float>());
}

void tr16_probe(torch::Tensor out, int64_t mode) {
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0,
                     (hipStream_t)at::cuda::getCurrentCUDAStream().stream(),
                     out.data_ptr<float>(), (int)mode);
}

// True when the geometry has a forward with the requested output form for
// this many same-geometry jobs (more than one job needs a grouped variant).
bool conv_fwd_supported(int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW,
                        int64_t S, int64_t COUT, bool u8, bool chw_out,
                        int64_t njobs) {
  const ConvEntry* e = find_conv(H, W, C, KH, KW, S, COUT, u8);
  if (!e || njobs < 1 || njobs > kMaxConvJobs) return false;
  if (njobs > 1) return (chw_out ? e->grouped_chw : e->grouped) != nullptr;
  return (chw_out ? e->fwd_chw : e->fwd) != nullptr;
}

// Fused conv + bias + ReLU forward for 1..kMaxConvJobs jobs of one geometry
// and batch size in a single launch (see conv_fwd_grouped_kernel).
// ins: (N,C,H,W) logical, channels_last, uint8 (dequant fused) or bf16;
// weights: (COUT,C,KH,KW) logical channels_last bf16; biases: empty, or one
// (COUT) bf16 tensor per job; outs: (N,COUT,P,Q) logical channels_last bf16,
// or with chw_out the flatten-fused 2-D (N, COUT*P*Q) in logical-NCHW order.
void conv_fwd_grouped(std::vector<torch::Tensor> ins,
                      std::vector<torch::Tensor> weights,
                      std::vector<torch::Tensor> biases,
                      std::vector<torch::Tensor> outs, int64_t stride,
                      bool chw_out) {
  const size_t njobs = ins.size();
  TORCH_CHECK(njobs >= 1 && njobs <= kMaxConvJobs, "1..", kMaxConvJobs,
              " conv jobs per launch");
  TORCH_CHECK(weights.size() == njobs && outs.size() == njobs &&
                  (biases.empty() || biases.size() == njobs),
              "conv_fwd_grouped wants one weight, output and bias per job");
  const Geom g = geom_of(ins[0], weights[0], stride);
  const ConvEntry* e = find_geom(kConvs, g);
  TORCH_CHECK(e, "no fused conv kernel for this geometry: ", g.H, "x", g.W,
              "x", g.C, " k", g.KH, "x", g.KW, " s", g.S, " -> ", g.COUT,
              " u8=", g.u8);
  launch_conv_fwd(*e, ins, weights, biases, outs, chw_out);
}

// Run a specific tuning variant (tools/gpu_conv_tune.py); returns false if
// the variant index does not match the geometry.
bool conv_fwd_variant(torch::Tensor in, torch::Tensor weight,
                      torch::Tensor bias, torch::Tensor out, int64_t stride,
                      int64_t variant) {
  if (variant < 0 || variant >= (int64_t)std::size(kVariants)) return false;
  const ConvEntry& e = kVariants[variant];
  if (!(e.g == geom_of(in, weight, stride))) return false;
  launch_conv_fwd(e, {in}, {weight}, {bias}, {out}, false);
  return true;
}

bool conv_wrw_supported(int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW,
                        int64_t S, int64_t COUT, bool u8) {
  const ConvEntry* e = find_conv(H, W, C, KH, KW, S, COUT, u8);
  return e && e->wrw;
}

namespace {

// a checked wrw call: table entry and row count
struct WrwCall {
  const ConvEntry* L;
  int64_t N, COUT;
  int M;
};

WrwCall check_wrw_inputs(const torch::Tensor& in, const torch::Tensor& gout,
                         int64_t stride) {
  TORCH_CHECK(in.dim() == 4 && gout.dim() == 4 && stride >= 1,
              "conv_wrw wants 4-D in and gout and a positive stride");
  const int64_t N = in.size(0), C = in.size(1), H = in.size(2), W = in.size(3);
  const int64_t COUT = gout.size(1), P = gout.size(2), Q = gout.size(3);
  const bool u8 = in.scalar_type() == torch::kUInt8;
  // table geometries have no ragged last window (make_conv asserts it), so
  // gout's extent fixes the kernel extent
  const ConvEntry* L =
      find_conv(H, W, C, H - (P - 1) * stride, W - (Q - 1) * stride, stride,
                COUT, u8);
  TORCH_CHECK(L && L->wrw, "no wrw kernel for this geometry");
  check_nhwc(in, u8 ? torch::kUInt8 : kBF16, N, C, H, W, "conv_wrw in");
  check_nhwc(gout, kBF16, N, COUT, P, Q, "conv_wrw gout (in's batch)");
  // 16-byte pieces of both
  TORCH_CHECK((uintptr_t)in.data_ptr() % 16 == 0 &&
                  (uintptr_t)gout.data_ptr() % 16 == 0,
              "conv_wrw: misaligned tensor");
  return WrwCall{L, N, COUT, checked_rows(N * P * Q, "conv_wrw")};
}

// What wrw_reduce_block dereferences for one job, checked: part (planes,
// n_elem + kPlanePad) fp32; gw n_elem elements of `dtype`, dense in (cout,
// kh, kw, c) order; b_part (b_planes, cout) fp32 and gb (cout) of gw's
// dtype, or both empty.
struct FoldJob {
  int planes, n_elem, b_planes, cout;
  bool bias;
};

// the output half of check_fold_job: planes and b_planes stay 0
FoldJob check_fold_out(const torch::Tensor& gw, const torch::Tensor& gb,
                       at::ScalarType dtype) {
  TORCH_CHECK(gw.defined(), "wrw fold gw is undefined");
  TORCH_CHECK(dtype == kBF16 || dtype == torch::kFloat32,
              "wrw fold writes fp32 or bf16");
  check_dev(gw, dtype, "wrw fold gw");
  TORCH_CHECK(gw.is_contiguous() ||
                  (gw.dim() == 4 &&
                   gw.is_contiguous(at::MemoryFormat::ChannelsLast)),
              "wrw fold gw must be dense in (cout, kh, kw, c) order");
  const int64_t n_elem = gw.numel();
  TORCH_CHECK(n_elem > 0 && n_elem % 64 == 0 && n_elem < ((int64_t)1 << 30),
              "wrw fold gw must hold a positive multiple of 64 elements");
  TORCH_CHECK((uintptr_t)gw.data_ptr() % 16 == 0, "wrw fold gw is misaligned");
  FoldJob j{0, (int)n_elem, 0, 0, gb.defined() && gb.numel() > 0};
  if (j.bias) {
    const int64_t cout = gb.numel();
    TORCH_CHECK(cout <= 256 && 256 % cout == 0,
                "wrw fold bias: cout must divide 256");
    check_rows(gb, dtype, {cout}, "wrw fold gb");
    TORCH_CHECK(gb.device() == gw.device(), "wrw fold: tensors on two devices");
    j.cout = (int)cout;
  }
  return j;
}

FoldJob check_fold_job(const torch::Tensor& part, int64_t mb,
                       const torch::Tensor& b_part, const torch::Tensor& gw,
                       const torch::Tensor& gb, at::ScalarType dtype) {
  FoldJob j = check_fold_out(gw, gb, dtype);
  const int64_t n_elem = j.n_elem;
  TORCH_CHECK(mb >= 1 && mb < ((int64_t)1 << 20), "wrw fold wants >= 1 plane");
  check_rows(part, torch::kFloat32, {mb, n_elem + kPlanePad},
             "wrw fold partial planes");
  TORCH_CHECK((uintptr_t)part.data_ptr() % 16 == 0,
              "wrw fold partial planes are misaligned");
  TORCH_CHECK(part.device() == gw.device(), "wrw fold: tensors on two devices");
  j.planes = (int)mb;
  const bool has_b_part = b_part.defined() && b_part.numel() > 0;
  TORCH_CHECK(j.bias == has_b_part,
              "wrw fold wants b_part and gb together or neither");
  if (j.bias) {
    const int64_t cout = j.cout;
    TORCH_CHECK(b_part.dim() == 2 && b_part.size(0) >= 1 &&
                    b_part.size(0) < ((int64_t)1 << 20),
                "wrw fold b_part must be (b_planes, cout)");
    check_rows(b_part, torch::kFloat32, {b_part.size(0), cout},
               "wrw fold b_part");
    TORCH_CHECK(b_part.device() == gw.device(),
                "wrw fold: tensors on two devices");
    j.b_planes = (int)b_part.size(0);
  }
  return j;
}

// m-slices of a call: scale the m-grid with the batch — R2D2/IMPALA run
// 8-20x Ape-X's row count through the same kernel (conv1 wrw measured 139 us
// at 1.02M rows with 512 blocks = 250 serial chunks per block); every
// m-slice costs one partial plane of write + read traffic
int wrw_mblocks(const ConvEntry& L, int M) {
  const int n_chunks = (M + 31) / 32;
  int mb = (n_chunks > 8192 ? 2048 : 512) / L.ktiles;
  if (mb > n_chunks) mb = n_chunks;
  if (mb < 1) mb = 1;
  return mb;
}

// The wrw launches of a checked call: per-m-slice partial planes (every
// (ktile, m-slice) block writes its whole 64 x COUT tile, so no zero-fill)
// and, with want_bias, colsum_bf16_kernel's kColsumBlocks x COUT column-sum
// partials of gout.
struct WrwPartials {
  torch::Tensor part, b_part;
  int mb;
};

WrwPartials launch_wrw_partials(const WrwCall& c, const torch::Tensor& in,
                                const torch::Tensor& gout, bool want_bias) {
  const ConvEntry& L = *c.L;
  const int mb = wrw_mblocks(L, c.M);
  const int64_t n_elem = c.COUT * L.g.K();
  const auto f32 = gout.options().dtype(torch::kFloat32);
  WrwPartials r;
  r.mb = mb;
  r.part = torch::empty({(int64_t)mb, n_elem + kPlanePad}, f32);
  auto st = cur_stream();
  hipLaunchKernelGGL(L.wrw, dim3(L.ktiles, mb), dim3(256), L.wrw_lds_bytes, st,
                     (const void*)in.data_ptr(),
                     (const __bf16*)gout.data_ptr(), r.part.data_ptr<float>(),
                     (int)c.N, mb);
  if (want_bias) {
    r.b_part = torch::empty({(int64_t)kColsumBlocks, c.COUT}, f32);
    hipLaunchKernelGGL(L.colsum, dim3(kColsumBlocks), dim3(256), 0, st,
                       (const __bf16*)gout.data_ptr(), (int64_t)c.M,
                       r.b_part.data_ptr<float>());
  }
  return r;
}

// wrw_reduce_grouped_kernel over checked jobs
template <typename OutT>
void launch_fold_grouped(const std::vector<FoldJob>& jobs,
                         const std::vector<torch::Tensor>& parts,
                         const std::vector<torch::Tensor>& b_parts,
                         const std::vector<torch::Tensor>& gws,
                         const std::vector<torch::Tensor>& gbs) {
  WrwFoldJobs<OutT> t{};
  int blocks = 0;
  for (size_t j = 0; j < jobs.size(); ++j) {
    t.part[j] = parts[j].data_ptr<float>();
    t.out[j] = (OutT*)gws[j].data_ptr();
    t.b_part[j] = jobs[j].bias ? b_parts[j].data_ptr<float>() : nullptr;
    t.b_out[j] = jobs[j].bias ? (OutT*)gbs[j].data_ptr() : nullptr;
    t.planes[j] = jobs[j].planes;
    t.n_elem[j] = jobs[j].n_elem;
    t.b_planes[j] = jobs[j].b_planes;
    t.cout[j] = jobs[j].cout;
    blocks += jobs[j].n_elem / 64 + (jobs[j].bias ? 1 : 0);
    t.end_block[j] = blocks;
  }
  hipLaunchKernelGGL(wrw_reduce_grouped_kernel<OutT>, dim3(blocks), dim3(256),
                     0, cur_stream(), t, (int)jobs.size());
}

}  // namespace

// in: (N,C,H,W) channels_last u8/bf16; gout: (N,COUT,P,Q) channels_last bf16
// (already relu-masked); gw_ws: (COUT, KH*KW*C) fp32 and gb_ws: (COUT) fp32
// (or empty), both fully overwritten. bf16 gw_ws/gb_ws are the gradients
// themselves: gw_ws then holds COUT*KH*KW*C elements in (cout, kh, kw, c)
// memory order (a channels_last weight-shaped tensor or its flat view).
// = conv_wrw_partials + a one-job wrw_fold_grouped.
void conv_wrw(torch::Tensor in, torch::Tensor gout, torch::Tensor gw_ws,
              torch::Tensor gb_ws, int64_t stride) {
  const WrwCall c = check_wrw_inputs(in, gout, stride);
  // the fold's outputs, before the first launch
  TORCH_CHECK(gw_ws.defined(), "conv_wrw gw_ws is undefined");
  const bool bias = check_fold_out(gw_ws, gb_ws, gw_ws.scalar_type()).bias;
  TORCH_CHECK(gw_ws.numel() == c.COUT * c.L->g.K(), "gw_ws shape mismatch");
  if (bias)
    check_rows(gb_ws, gw_ws.scalar_type(), {c.COUT}, "conv_wrw gb_ws");
  TORCH_CHECK(gw_ws.device() == gout.device(), "conv_wrw: two devices");
  WrwPartials r = launch_wrw_partials(c, in, gout, bias);
  const FoldJob job = check_fold_job(r.part, r.mb, r.b_part, gw_ws, gb_ws,
                                     gw_ws.scalar_type());
  if (gw_ws.scalar_type() == kBF16)
    launch_fold_grouped<__bf16>({job}, {r.part}, {r.b_part}, {gw_ws}, {gb_ws});
  else
    launch_fold_grouped<float>({job}, {r.part}, {r.b_part}, {gw_ws}, {gb_ws});
}

// The wrw launches alone: (part, mb, b_part) for wrw_fold_grouped; b_part is
// an empty tensor without want_bias.
std::tuple<torch::Tensor, int64_t, torch::Tensor> conv_wrw_partials(
    torch::Tensor in, torch::Tensor gout, int64_t stride, bool want_bias) {
  const WrwCall c = check_wrw_inputs(in, gout, stride);
  WrwPartials r = launch_wrw_partials(c, in, gout, want_bias);
  if (!want_bias) r.b_part = torch::empty({0}, r.part.options());
  return {r.part, (int64_t)r.mb, r.b_part};
}

// Ordered fold of 1..kMaxFoldJobs weight gradients in one launch. Job j:
// parts[j] (mbs[j], n_elem + plane pad) fp32 planes -> gws[j] (n_elem
// elements, fp32 or bf16, one dtype for all jobs); b_parts[j] (b_planes,
// cout) fp32 -> gbs[j] (cout) of the same dtype, or both empty for a job
// without bias. Every job is checked before the launch.
void wrw_fold_grouped(std::vector<torch::Tensor> parts,
                      std::vector<int64_t> mbs,
                      std::vector<torch::Tensor> b_parts,
                      std::vector<torch::Tensor> gws,
                      std::vector<torch::Tensor> gbs) {
  const size_t n = parts.size();
  TORCH_CHECK(n >= 1 && n <= (size_t)kMaxFoldJobs, "1..", kMaxFoldJobs,
              " fold jobs per launch");
  TORCH_CHECK(mbs.size() == n && b_parts.size() == n && gws.size() == n &&
                  gbs.size() == n,
              "wrw_fold_grouped wants one entry per job in every list");
  TORCH_CHECK(gws[0].defined(), "wrw fold gw is undefined");
  const at::ScalarType dtype = gws[0].scalar_type();
  std::vector<FoldJob> jobs;
  for (size_t j = 0; j < n; ++j) {
    jobs.push_back(
        check_fold_job(parts[j], mbs[j], b_parts[j], gws[j], gbs[j], dtype));
    TORCH_CHECK(gws[j].device() == gws[0].device(),
                "wrw fold: jobs on two devices");
  }
  if (dtype == kBF16)
    launch_fold_grouped<__bf16>(jobs, parts, b_parts, gws, gbs);
  else
    launch_fold_grouped<float>(jobs, parts, b_parts, gws, gbs);
}

int64_t wrw_plane_pad() { return kPlanePad; }

bool conv_dgrad_supported(int64_t H, int64_t W, int64_t C, int64_t KH,
                          int64_t KW, int64_t S, int64_t COUT) {
  return find_geom(kDgrad, Geom{H, W, C, KH, KW, S, COUT, false}) != nullptr;
}

// gout: (N,COUT,P,Q) logical channels_last bf16; weight (COUT,C,KH,KW)
// logical channels_last bf16; dx out (N,C,H,W) logical channels_last bf16;
// w_t workspace (C*KH*KW*COUT) bf16.
void conv_dgrad(torch::Tensor gout, torch::Tensor weight, torch::Tensor w_t,
                torch::Tensor dx, int64_t stride) {
  TORCH_CHECK(dx.dim() == 4 && weight.dim() == 4 && stride >= 1,
              "conv_dgrad wants 4-D dx and weight and a positive stride");
  const int64_t N = dx.size(0), C = dx.size(1), H = dx.size(2), W = dx.size(3);
  const int64_t COUT = weight.size(0), KH = weight.size(2), KW = weight.size(3);
  const DgradEntry* L =
      find_geom(kDgrad, Geom{H, W, C, KH, KW, stride, COUT, false});
  TORCH_CHECK(L, "no dgrad kernel for this geometry");
  check_nhwc(dx, kBF16, N, C, H, W, "conv_dgrad dx");
  check_nhwc(weight, kBF16, COUT, C, KH, KW, "conv_dgrad weight");
  check_nhwc(gout, kBF16, N, COUT, L->g.P(), L->g.Q(), "conv_dgrad gout");
  check_rows(w_t, kBF16, {weight.numel()}, "conv_dgrad w_t");
  const int M = checked_rows(N * H * W, "conv_dgrad");
  if (M == 0) return;
  auto stream = cur_stream();
  const int total = (int)weight.numel();
  hipLaunchKernelGGL(conv_w_transpose_kernel, dim3((total + 255) / 256),
                     dim3(256), 0, stream, (const __bf16*)weight.data_ptr(),
                     (__bf16*)w_t.data_ptr(), (int)(KH * KW), (int)C,
                     (int)COUT);
  const int rows_per_block = L->waves * L->rpw;
  const int blocks = (M + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL(L->fn, dim3(blocks), dim3(L->waves * 64), 0, stream,
                     (const __bf16*)gout.data_ptr(),
                     (const __bf16*)w_t.data_ptr(), (__bf16*)dx.data_ptr(),
                     (int)N);
}

// backward of the flatten-fused forward: gout2d / out2d are the (N, C*PQ)
// CHW-ordered grad and forward output, dst_nhwc the (N,C,P,Q) logical
// channels_last relu-masked grad.
void relu_mask_bwd_chw(torch::Tensor gout2d, torch::Tensor out2d,
                       torch::Tensor dst_nhwc, int64_t C, int64_t PQ) {
  TORCH_CHECK(gout2d.dim() == 2 && dst_nhwc.dim() == 4 && C >= 1 && PQ >= 1);
  const int64_t N = gout2d.size(0);
  check_rows(gout2d, kBF16, {N, C * PQ}, "relu_mask_bwd_chw gout");
  check_rows(out2d, kBF16, {N, C * PQ}, "relu_mask_bwd_chw out");
  TORCH_CHECK(dst_nhwc.size(2) * dst_nhwc.size(3) == PQ,
              "relu_mask_bwd_chw dst must have P*Q == ", PQ);
  check_nhwc(dst_nhwc, kBF16, N, C, dst_nhwc.size(2), dst_nhwc.size(3),
             "relu_mask_bwd_chw dst");
  const int64_t total = N * C * PQ;
  if (total == 0) return;
  int blocks = (int)std::min<int64_t>((total + 255) / 256, 2048);
  hipLaunchKernelGGL(relu_mask_bwd_chw_kernel, dim3(blocks), dim3(256), 0,
                     cur_stream(), (const __bf16*)gout2d.data_ptr(),
                     (const __bf16*)out2d.data_ptr(),
                     (__bf16*)dst_nhwc.data_ptr(), N, (int)C, (int)PQ);
}

bool linear_relu_supported(int64_t K, int64_t N) {
  return (K == 3136 && N == 1024);
}

// out(M, N) = relu(x(M, K) @ w(N, K)^T + b(N)), all bf16; b may be empty.
void linear_relu(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                 torch::Tensor out) {
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2);
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(linear_relu_supported(K, N), "no linear_relu instantiation");
  check_rows(x, kBF16, {M, K}, "linear_relu x");
  check_rows(w, kBF16, {N, K}, "linear_relu w");
  check_rows(out, kBF16, {M, N}, "linear_relu out");
  const __bf16* bp = opt_vec(b, N, "linear_relu bias");
  if (M == 0) return;
  dim3 grid((checked_rows(M, "linear_relu") + 31) / 32, N / 256);
  hipLaunchKernelGGL((linear_relu_kernel<3136, 1024, 256>), grid, dim3(256),
                     0, cur_stream(), (const __bf16*)x.data_ptr(),
                     (const __bf16*)w.data_ptr(), bp, (__bf16*)out.data_ptr(),
                     (int)M);
}

// a table geometry, or any H, W >= 1 at a (C, COUT) with a run-time entry
bool conv3x3p1_supported(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  return find_conv3(H, W, C, COUT) != nullptr ||
         find_conv3_hw(H, W, C, COUT) != nullptr;
}

// in: (N,C,H,W) logical channels_last bf16; weight: (COUT,C,3,3) logical
// channels_last bf16; bias: (COUT) bf16 or empty; residual: same shape and
// layout as out, or empty; out: (N,COUT,H,W) logical channels_last bf16.
// One launch on the current stream, no allocation, no sync (graph-safe).
// any_hw: run the run-time H, W kernel even at a table geometry (tests and
// tools/gpu_resconv_hw_bench.py).
void conv3x3p1_fwd(torch::Tensor in, torch::Tensor weight, torch::Tensor bias,
                   torch::Tensor residual, torch::Tensor out, bool relu_in,
                   bool relu_out, bool any_hw) {
  TORCH_CHECK(in.dim() == 4 && weight.dim() == 4);
  const int64_t COUT = weight.size(0);
  check_nhwc(weight, kBF16, COUT, in.size(1), 3, 3, "conv3x3p1_fwd weight");
  launch_conv3(in, (const __bf16*)weight.data_ptr(), nullptr, bias, residual,
               torch::Tensor(), out, COUT, relu_in, relu_out, any_hw,
               {"conv3x3p1_fwd input", "conv3x3p1_fwd output",
                "conv3x3p1_fwd bias", "conv3x3p1_fwd residual",
                "conv3x3p1_fwd mask"});
}

bool conv3x3p1_wrw_supported(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  const Conv3Launch* L = find_conv3(H, W, C, COUT);
  if (L) return L->wrw != nullptr;
  const Conv3HwLaunch* R = find_conv3_hw(H, W, C, COUT);
  return R && R->wrw;
}

namespace {
// What conv3x3p1_wrw launches for x (N,C,H,W) -> COUT: the entry (table
// first, then run-time; any_hw skips the table), its rows per pass, M and
// the m-grid from wrw_m_grid with that entry's residency figure. The
// launch and the conv3x3p1_wrw_plan query both take it from here.
struct Conv3WrwPlan {
  const Conv3Launch* L;
  const Conv3HwLaunch* R;
  int rows, M, resident, mb;
};

Conv3WrwPlan plan_conv3_wrw(int64_t N, int64_t H, int64_t W, int64_t C,
                            int64_t COUT, bool any_hw) {
  Conv3WrwPlan p{};
  p.L = any_hw ? nullptr : find_conv3(H, W, C, COUT);
  p.R = p.L ? nullptr : find_conv3_hw(H, W, C, COUT);
  TORCH_CHECK(p.L ? p.L->wrw != nullptr : p.R && p.R->wrw,
              "no 3x3 pad-1 wrw kernel for this geometry: ", H, "x", W, "x", C,
              " -> ", COUT);
  p.rows = p.L ? p.L->wrw_rows : p.R->wrw_rows;
  // the last pass's row numbers run past M by less than a pass
  p.M = checked_rows(N * H * W + p.rows, "conv3x3p1_wrw") - p.rows;
  p.resident = p.L ? wrw_resident_blocks(*p.L) : wrw_resident_blocks(*p.R);
  p.mb = wrw_m_grid((p.M + p.rows - 1) / p.rows,
                    (COUT * 9 * C + kPlanePad) * 4, p.resident);
  return p;
}
}  // namespace

// (m-blocks, rows per pass, resident blocks) of the conv3x3p1_wrw call on
// an x of this shape: the launch's own plan, for the tests that pin the
// summation order of the run-time path
std::tuple<int64_t, int64_t, int64_t> conv3x3p1_wrw_plan(
    int64_t N, int64_t H, int64_t W, int64_t C, int64_t COUT, bool any_hw) {
  const Conv3WrwPlan p = plan_conv3_wrw(N, H, W, C, COUT, any_hw);
  return {p.mb, p.rows, p.resident};
}

// x: (N,C,H,W) and gout: (N,COUT,H,W) logical channels_last bf16 (gout
// already relu-masked); gw: (COUT, 9C) fp32 workspace, or the bf16 gradient
// itself in (cout, kh, kw, c) memory order; gb: (COUT) of gw's dtype, or
// empty — conv_wrw's contracts. relu_in: the conv read relu(x). any_hw: as
// conv3x3p1_fwd's. The m-grid, and with it the summation order, follows
// the residency figure of the kernel that runs.
void conv3x3p1_wrw(torch::Tensor x, torch::Tensor gout, torch::Tensor gw,
                   torch::Tensor gb, bool relu_in, bool any_hw) {
  TORCH_CHECK(x.dim() == 4 && gout.dim() == 4,
              "conv3x3p1_wrw wants 4-D x and gout");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t COUT = gout.size(1);
  const Conv3WrwPlan plan = plan_conv3_wrw(N, H, W, C, COUT, any_hw);
  const Conv3Launch* L = plan.L;
  const Conv3HwLaunch* R = plan.R;
  check_nhwc(x, kBF16, N, C, H, W, "conv3x3p1_wrw x");
  check_nhwc(gout, kBF16, N, COUT, H, W, "conv3x3p1_wrw gout (x's batch)");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)gout.data_ptr() % 16 == 0,
              "conv3x3p1_wrw: misaligned tensor");
  const bool bf16_out = gw.scalar_type() == kBF16;
  check_dev(gw, bf16_out ? kBF16 : torch::kFloat32, "conv3x3p1_wrw gw");
  TORCH_CHECK(gw.is_contiguous() ||
                  (gw.dim() == 4 &&
                   gw.is_contiguous(at::MemoryFormat::ChannelsLast)),
              "conv3x3p1_wrw gw must be dense in (cout, kh, kw, c) order");
  const int64_t n_elem = COUT * 9 * C;
  TORCH_CHECK(gw.numel() == n_elem, "conv3x3p1_wrw gw must hold ", n_elem,
              " elements, got ", gw.numel());
  const bool bias = gb.defined() && gb.numel() > 0;
  if (bias) check_rows(gb, gw.scalar_type(), {COUT}, "conv3x3p1_wrw gb");
  const int M = plan.M, mb = plan.mb;
  const auto f32 = gw.options().dtype(torch::kFloat32);
  auto part = torch::empty({(int64_t)mb, n_elem + kPlanePad}, f32);
  if (L)
    hipLaunchKernelGGL(L->wrw, dim3(mb), dim3(256), L->wrw_lds_bytes,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (const __bf16*)gout.data_ptr(), part.data_ptr<float>(),
                       (int)N, mb, relu_in ? 1 : 0);
  else
    hipLaunchKernelGGL(R->wrw, dim3(mb), dim3(256), R->wrw_lds_bytes,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (const __bf16*)gout.data_ptr(), part.data_ptr<float>(),
                       (int)N, mb, relu_in ? 1 : 0, (int)H, (int)W);
  launch_wrw_fold(part, mb, gout, M, COUT, L ? L->colsum : R->colsum, gw, gb,
                  bias);
}

// Input gradient of the conv (x -> out, weight (COUT,C,3,3)) through the
// forward kernel at the mirrored geometry: gx = conv3x3p1(gout, W').
// gout: (N,COUT,H,W); weight: (COUT,C,3,3); w_flip_ws: COUT*C*9 bf16
// workspace (overwritten with W'); gx: (N,C,H,W); mask_x: empty, or the
// conv's input x — gx is then zeroed where x <= 0 (relu_in backward). All
// logical channels_last bf16. Two launches, no allocation (graph-safe).
// any_hw: as conv3x3p1_fwd's.
void conv3x3p1_dgrad(torch::Tensor gout, torch::Tensor weight,
                     torch::Tensor w_flip_ws, torch::Tensor gx,
                     torch::Tensor mask_x, bool any_hw) {
  TORCH_CHECK(gout.dim() == 4 && weight.dim() == 4 && gx.dim() == 4,
              "conv3x3p1_dgrad wants 4-D gout, weight and gx");
  const int64_t COUT = weight.size(0), C = weight.size(1);
  TORCH_CHECK(gout.size(1) == COUT, "conv3x3p1_dgrad: gout has ",
              gout.size(1), " channels, weight ", COUT);
  TORCH_CHECK(gx.size(0) == gout.size(0), "conv3x3p1_dgrad: batch mismatch");
  check_nhwc(weight, kBF16, COUT, C, 3, 3, "conv3x3p1_dgrad weight");
  check_rows(w_flip_ws, kBF16, {weight.numel()}, "conv3x3p1_dgrad w_flip_ws");
  launch_conv3(gout, (const __bf16*)w_flip_ws.data_ptr(),
               (const __bf16*)weight.data_ptr(), torch::Tensor(),
               torch::Tensor(), mask_x, gx, C, false, false, any_hw,
               {"conv3x3p1_dgrad gout", "conv3x3p1_dgrad gx",
                "conv3x3p1_dgrad bias", "conv3x3p1_dgrad residual",
                "conv3x3p1_dgrad mask_x"});
}

bool conv3x3c4_supported(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  return find_stem(H, W, C, COUT) != nullptr;
}

bool conv3x3c4_wrw_supported(int64_t H, int64_t W, int64_t C, int64_t COUT) {
  const StemLaunch* L = find_stem(H, W, C, COUT);
  return L && L->wrw;
}

// the run-time stem kernels: any H, W >= 1 at this (C, COUT)
bool conv3x3c4_hw_supported(int64_t C, int64_t COUT) {
  return find_stem_hw(C, COUT) != nullptr;
}

namespace {
// The stem entry of a call: `table` (conv3x3c4_fwd / _wrw) takes
// kStemLaunches and rejects every other geometry; otherwise (the _hw
// bindings) the (C, COUT) run-time entry at any H, W >= 1, table geometry
// included. An error names the argument the geometry fails on.
struct StemPick {
  const StemLaunch* L;
  const StemHwLaunch* R;
  int waves() const { return L ? L->waves : R->waves; }
  int rpw() const { return L ? L->rpw : R->rpw; }
  int wrw_rows() const { return L ? L->wrw_rows : R->wrw_rows; }
};

StemPick stem_for(const torch::Tensor& x, int64_t COUT, bool table,
                  const std::string& x_name, const std::string& cout_name) {
  const int64_t C = x.size(1), H = x.size(2), W = x.size(3);
  bool x_known = false;
  if (table) {
    if (const StemLaunch* L = find_stem(H, W, C, COUT)) return {L, nullptr};
    for (const auto& l : kStemLaunches)
      x_known = x_known || (l.H == H && l.W == W && l.C == C);
  } else {
    if (H >= 1 && W >= 1)
      if (const StemHwLaunch* R = find_stem_hw(C, COUT)) return {nullptr, R};
    for (const auto& l : kStemHwLaunches)
      x_known = x_known || (H >= 1 && W >= 1 && l.C == C);
  }
  // the table bindings keep their wording
  const char* no = table ? ": no stem conv kernel for "
                         : ": no stem conv kernel for this geometry: ";
  TORCH_CHECK(x_known, x_name, no, H, "x", W, "x", C);
  TORCH_CHECK(false, cout_name, no, H, "x", W, "x", C, " -> ", COUT);
  return {nullptr, nullptr};
}

// rows per pass, M and m-grid of a stem weight gradient on entry S:
// conv3x3p1_wrw's three rules with the residency figure of the kernel that
// runs. The launch and the conv3x3c4_wrw_plan query both take it from here.
struct StemWrwPlan {
  int rows, M, resident, mb;
};

StemWrwPlan plan_stem_wrw(const StemPick& S, int64_t N, int64_t H, int64_t W,
                          const char* who) {
  StemWrwPlan p{};
  p.rows = S.wrw_rows();
  // the last pass's row numbers run past M by less than a pass
  p.M = checked_rows(N * H * W + p.rows, who) - p.rows;
  p.resident = S.L ? wrw_resident_blocks(*S.L) : wrw_resident_blocks(*S.R);
  p.mb = wrw_m_grid((p.M + p.rows - 1) / p.rows,
                    (StemGeom::COUT * StemGeom::K + kPlanePad) * 4, p.resident);
  return p;
}

// who: the binding's name, the prefix of every argument name in an error
void stem_fwd(const torch::Tensor& x, const torch::Tensor& weight,
              const torch::Tensor& bias, const torch::Tensor& out, bool table,
              const std::string& who) {
  TORCH_CHECK(x.dim() == 4 && weight.dim() == 4, who,
              " wants 4-D x and weight");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t COUT = weight.size(0);
  const std::string xn = who + " x", wn = who + " weight", on = who + " out",
                    bn = who + " bias";
  const StemPick S = stem_for(x, COUT, table, xn, wn);
  check_nhwc(x, kBF16, N, C, H, W, xn.c_str());
  check_nhwc(weight, kBF16, COUT, C, 3, 3, wn.c_str());
  check_nhwc(out, kBF16, N, COUT, H, W, on.c_str());
  TORCH_CHECK(out.data_ptr() != x.data_ptr(), on, " must not alias x");
  // 8-byte pieces of x, weight and out
  TORCH_CHECK((uintptr_t)x.data_ptr() % 8 == 0, xn, " is misaligned");
  TORCH_CHECK((uintptr_t)weight.data_ptr() % 8 == 0, wn, " is misaligned");
  TORCH_CHECK((uintptr_t)out.data_ptr() % 8 == 0, on, " is misaligned");
  const __bf16* bias_ptr = opt_vec(bias, COUT, bn.c_str());
  const int M = checked_rows(N * H * W, on.c_str());
  if (M == 0) return;
  const int rows_per_block = S.waves() * S.rpw();
  const int blocks = (M + rows_per_block - 1) / rows_per_block;
  if (S.L)
    hipLaunchKernelGGL(S.L->fwd, dim3(blocks), dim3(S.L->waves * 64),
                       S.L->lds_bytes, cur_stream(),
                       (const __bf16*)x.data_ptr(),
                       (const __bf16*)weight.data_ptr(), bias_ptr,
                       (__bf16*)out.data_ptr(), (int)N);
  else
    hipLaunchKernelGGL(S.R->fwd, dim3(blocks), dim3(S.R->waves * 64),
                       S.R->lds_bytes, cur_stream(),
                       (const __bf16*)x.data_ptr(),
                       (const __bf16*)weight.data_ptr(), bias_ptr,
                       (__bf16*)out.data_ptr(), (int)N, (int)H, (int)W);
}

void stem_wrw(const torch::Tensor& x, const torch::Tensor& gout,
              torch::Tensor& gw, torch::Tensor& gb, bool table,
              const std::string& who) {
  TORCH_CHECK(x.dim() == 4 && gout.dim() == 4, who, " wants 4-D x and gout");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int64_t COUT = gout.size(1);
  const std::string xn = who + " x", gn = who + " gout", gwn = who + " gw",
                    gbn = who + " gb";
  const StemPick S = stem_for(x, COUT, table, xn, gn);
  check_nhwc(x, kBF16, N, C, H, W, xn.c_str());
  check_nhwc(gout, kBF16, N, COUT, H, W, (gn + " (x's batch)").c_str());
  // 8-byte pieces of x, 16-byte pieces of gout, 16-byte stores to gw
  TORCH_CHECK((uintptr_t)x.data_ptr() % 8 == 0, xn, " is misaligned");
  TORCH_CHECK((uintptr_t)gout.data_ptr() % 16 == 0, gn, " is misaligned");
  TORCH_CHECK(gw.defined(), gwn, " is undefined");
  const bool bf16_out = gw.scalar_type() == kBF16;
  check_dev(gw, bf16_out ? kBF16 : torch::kFloat32, gwn.c_str());
  TORCH_CHECK(gw.is_contiguous() ||
                  (gw.dim() == 4 &&
                   gw.is_contiguous(at::MemoryFormat::ChannelsLast)),
              gwn, " must be dense in (cout, kh, kw, c) order");
  const int64_t n_elem = COUT * 9 * C;
  TORCH_CHECK(gw.numel() == n_elem, gwn, " must hold ", n_elem,
              " elements, got ", gw.numel());
  TORCH_CHECK((uintptr_t)gw.data_ptr() % 16 == 0, gwn, " is misaligned");
  const bool bias = gb.defined() && gb.numel() > 0;
  if (bias) check_rows(gb, gw.scalar_type(), {COUT}, gbn.c_str());
  const StemWrwPlan plan = plan_stem_wrw(S, N, H, W, xn.c_str());
  const int M = plan.M, mb = plan.mb;
  const auto f32 = gw.options().dtype(torch::kFloat32);
  auto part = torch::empty({(int64_t)mb, n_elem + kPlanePad}, f32);
  if (S.L)
    hipLaunchKernelGGL(S.L->wrw, dim3(mb), dim3(256), S.L->wrw_lds_bytes,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (const __bf16*)gout.data_ptr(), part.data_ptr<float>(),
                       (int)N, mb);
  else
    hipLaunchKernelGGL(S.R->wrw, dim3(mb), dim3(256), S.R->wrw_lds_bytes,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (const __bf16*)gout.data_ptr(), part.data_ptr<float>(),
                       (int)N, mb, (int)H, (int)W);
  launch_wrw_fold(part, mb, gout, M, COUT, S.L ? S.L->colsum : S.R->colsum,
                  gw, gb, bias);
}
}  // namespace

// x: (N,4,84,84) logical channels_last bf16; weight: (16,4,3,3) logical
// channels_last bf16; bias: (16) bf16 or empty; out: (N,16,84,84) logical
// channels_last bf16. One launch on the current stream, no allocation, no
// sync (graph-safe). The table kernel: 84x84 only.
void conv3x3c4_fwd(torch::Tensor x, torch::Tensor weight, torch::Tensor bias,
                   torch::Tensor out) {
  stem_fwd(x, weight, bias, out, true, "conv3x3c4_fwd");
}

// conv3x3c4_fwd at any H, W >= 1 (84x84 included) on the run-time kernel
void conv3x3c4_fwd_hw(torch::Tensor x, torch::Tensor weight,
                      torch::Tensor bias, torch::Tensor out) {
  stem_fwd(x, weight, bias, out, false, "conv3x3c4_fwd_hw");
}

// x: (N,4,84,84) and gout: (N,16,84,84) logical channels_last bf16; gw:
// (16, 36) fp32 workspace, or the bf16 gradient itself dense in (cout, kh,
// kw, c) order; gb: (16) of gw's dtype, or empty — conv3x3p1_wrw's
// contracts. The only allocation is the partial planes (and the bias
// partials of the fold).
void conv3x3c4_wrw(torch::Tensor x, torch::Tensor gout, torch::Tensor gw,
                   torch::Tensor gb) {
  stem_wrw(x, gout, gw, gb, true, "conv3x3c4_wrw");
}

// (m-blocks, rows per pass, resident blocks) of the stem weight gradient on
// N images of HxW: conv3x3c4_wrw_hw's plan (hw) or conv3x3c4_wrw's
std::tuple<int64_t, int64_t, int64_t> conv3x3c4_wrw_plan(int64_t N, int64_t H,
                                                         int64_t W, bool hw) {
  const StemLaunch* L =
      hw ? nullptr : find_stem(H, W, StemGeom::C, StemGeom::COUT);
  const StemHwLaunch* R =
      hw && H >= 1 && W >= 1 ? find_stem_hw(StemGeom::C, StemGeom::COUT)
                             : nullptr;
  TORCH_CHECK(L || R, "conv3x3c4_wrw_plan: no stem conv kernel for this "
              "geometry: ", H, "x", W);
  const StemWrwPlan p =
      plan_stem_wrw(StemPick{L, R}, N, H, W, "conv3x3c4_wrw_plan");
  return {p.mb, p.rows, p.resident};
}

// conv3x3c4_wrw at any H, W >= 1 (84x84 included) on the run-time kernel
void conv3x3c4_wrw_hw(torch::Tensor x, torch::Tensor gout, torch::Tensor gw,
                      torch::Tensor gb) {
  stem_wrw(x, gout, gw, gb, false, "conv3x3c4_wrw_hw");
}

bool maxpool3x3s2_supported(int64_t H, int64_t W, int64_t C) {
  return H >= 1 && W >= 1 && C >= 16 && C % 16 == 0;
}

// x: (N,C,H,W), out: (N,C,P,Q) logical channels_last bf16; idx: uint8 of
// out's shape and layout (winning tap kh*3 + kw), or empty: no index plane
// is written (a forward that needs no gradient). One launch, no allocation.
void maxpool3x3s2_fwd(torch::Tensor x, torch::Tensor out, torch::Tensor idx) {
  TORCH_CHECK(x.dim() == 4, "maxpool3x3s2_fwd wants a 4-D x");
  const int64_t N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(maxpool3x3s2_supported(H, W, C),
              "no 3x3 s2 max-pool kernel for this geometry: ", H, "x", W, "x",
              C);
  const int64_t P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  check_nhwc(x, kBF16, N, C, H, W, "maxpool3x3s2_fwd x");
  check_nhwc(out, kBF16, N, C, P, Q, "maxpool3x3s2_fwd out");
  const bool with_idx = idx.defined() && idx.numel() > 0;
  if (with_idx)
    check_nhwc(idx, torch::kUInt8, N, C, P, Q, "maxpool3x3s2_fwd idx");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 &&
                  (uintptr_t)out.data_ptr() % 16 == 0 &&
                  (!with_idx || (uintptr_t)idx.data_ptr() % 16 == 0),
              "maxpool3x3s2_fwd: misaligned tensor");
  // the kernel numbers input pixels with int as well
  checked_rows(N * H * W, "maxpool3x3s2_fwd");
  const int lanes = checked_rows(N * P * Q * (C / 16), "maxpool3x3s2_fwd");
  if (lanes == 0) return;
  const dim3 grid((unsigned)(((int64_t)lanes + 255) / 256));
  if (with_idx)
    hipLaunchKernelGGL(maxpool3x3s2_fwd_kernel<true>, grid, dim3(256), 0,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (__bf16*)out.data_ptr(), (uint8_t*)idx.data_ptr(),
                       lanes, (int)H, (int)W, (int)P, (int)Q, (int)(C / 16));
  else
    hipLaunchKernelGGL(maxpool3x3s2_fwd_kernel<false>, grid, dim3(256), 0,
                       cur_stream(), (const __bf16*)x.data_ptr(),
                       (__bf16*)out.data_ptr(), (uint8_t*)nullptr, lanes,
                       (int)H, (int)W, (int)P, (int)Q, (int)(C / 16));
}

// gout: (N,C,P,Q) bf16 and idx: uint8 of the same shape, as the forward
// left them; gx: (N,C,H,W) bf16, every element written. All logical
// channels_last. One launch, no allocation, no atomics.
void maxpool3x3s2_bwd(torch::Tensor gout, torch::Tensor idx,
                      torch::Tensor gx) {
  TORCH_CHECK(gx.dim() == 4, "maxpool3x3s2_bwd wants a 4-D gx");
  const int64_t N = gx.size(0), C = gx.size(1), H = gx.size(2), W = gx.size(3);
  TORCH_CHECK(maxpool3x3s2_supported(H, W, C),
              "no 3x3 s2 max-pool kernel for this geometry: ", H, "x", W, "x",
              C);
  const int64_t P = (H - 1) / 2 + 1, Q = (W - 1) / 2 + 1;
  check_nhwc(gout, kBF16, N, C, P, Q, "maxpool3x3s2_bwd gout");
  check_nhwc(idx, torch::kUInt8, N, C, P, Q, "maxpool3x3s2_bwd idx");
  check_nhwc(gx, kBF16, N, C, H, W, "maxpool3x3s2_bwd gx");
  TORCH_CHECK((uintptr_t)gout.data_ptr() % 16 == 0 &&
                  (uintptr_t)idx.data_ptr() % 16 == 0 &&
                  (uintptr_t)gx.data_ptr() % 16 == 0,
              "maxpool3x3s2_bwd: misaligned tensor");
  const int lanes = checked_rows(N * H * W * (C / 16), "maxpool3x3s2_bwd");
  if (lanes == 0) return;
  const dim3 grid((unsigned)(((int64_t)lanes + 255) / 256));
  hipLaunchKernelGGL(maxpool3x3s2_bwd_kernel, grid, dim3(256), 0, cur_stream(),
                     (const __bf16*)gout.data_ptr(),
                     (const uint8_t*)idx.data_ptr(), (__bf16*)gx.data_ptr(),
                     lanes, (int)H, (int)W, (int)P, (int)Q, (int)(C / 16));
}

void register_conv(pybind11::module_& m) {
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA fragment-map probe");
  m.def("tr16_probe", &tr16_probe);
  m.def("conv_fwd_grouped", &conv_fwd_grouped,
        "fused NHWC bf16 MFMA conv fwd (+dequant on u8 input, bias, ReLU, "
        "optional flatten-fused CHW out) for 1..4 same-geometry jobs in one "
        "launch");
  m.def("conv_fwd_supported", &conv_fwd_supported);
  m.def("conv_fwd_variant", &conv_fwd_variant, "tuning-variant conv fwd");
  m.def("conv_wrw", &conv_wrw,
        "MFMA conv weight-grad; gw/gb are fp32 workspaces or bf16 grads");
  m.def("conv_wrw_supported", &conv_wrw_supported);
  m.def("conv_wrw_partials", &conv_wrw_partials,
        "wrw launch only -> (part, mb, b_part) for wrw_fold_grouped");
  m.def("wrw_fold_grouped", &wrw_fold_grouped,
        "ordered fold of up to 4 weight gradients in one launch");
  m.def("wrw_plane_pad", &wrw_plane_pad);
  m.def("conv_dgrad", &conv_dgrad,
        "MFMA conv data-grad (masked-tap gather, pre-transposed weights)");
  m.def("conv_dgrad_supported", &conv_dgrad_supported);
  m.def("relu_mask_bwd_chw", &relu_mask_bwd_chw,
        "relu-mask + CHW->NHWC transpose (backward of the fused flatten)");
  m.def("linear_relu", &linear_relu,
        "fused Linear+bias+ReLU fwd (own MFMA GEMM, LDS-staged W)");
  m.def("linear_relu_supported", &linear_relu_supported);
  namespace py = pybind11;
  m.def("conv3x3p1_fwd", &conv3x3p1_fwd,
        "MFMA 3x3 s1 pad-1 NHWC bf16 conv fwd (+relu_in, bias, residual, "
        "relu_out); any_hw forces the run-time H, W kernel",
        py::arg("input"), py::arg("weight"), py::arg("bias"),
        py::arg("residual"), py::arg("out"), py::arg("relu_in"),
        py::arg("relu_out"), py::arg("any_hw") = false);
  m.def("conv3x3p1_supported", &conv3x3p1_supported);
  m.def("conv3x3p1_wrw", &conv3x3p1_wrw,
        "MFMA 3x3 s1 pad-1 weight-grad (+relu_in); gw/gb are fp32 workspaces "
        "or bf16 grads",
        py::arg("x"), py::arg("gout"), py::arg("gw"), py::arg("gb"),
        py::arg("relu_in"), py::arg("any_hw") = false);
  m.def("conv3x3p1_wrw_supported", &conv3x3p1_wrw_supported);
  m.def("conv3x3p1_dgrad", &conv3x3p1_dgrad,
        "3x3 s1 pad-1 input-grad: weight flip + the forward kernel at the "
        "mirrored geometry (+relu_in mask in the epilogue)",
        py::arg("gout"), py::arg("weight"), py::arg("w_flip_ws"),
        py::arg("gx"), py::arg("mask_x"), py::arg("any_hw") = false);
  m.def("conv3x3c4_fwd", &conv3x3c4_fwd,
        "MFMA 3x3 s1 pad-1 NHWC bf16 stem conv fwd (84x84, C=4 -> 16; bias)");
  m.def("conv3x3c4_supported", &conv3x3c4_supported);
  m.def("conv3x3c4_wrw", &conv3x3c4_wrw,
        "MFMA stem-conv weight-grad, ordered planes; gw/gb are fp32 "
        "workspaces or bf16 grads");
  m.def("conv3x3c4_wrw_supported", &conv3x3c4_wrw_supported);
  m.def("conv3x3c4_fwd_hw", &conv3x3c4_fwd_hw,
        "conv3x3c4_fwd at any H, W >= 1: the run-time H, W stem kernel");
  m.def("conv3x3c4_wrw_hw", &conv3x3c4_wrw_hw,
        "conv3x3c4_wrw at any H, W >= 1: the run-time H, W stem kernel");
  m.def("conv3x3c4_hw_supported", &conv3x3c4_hw_supported);
  m.def("conv3x3p1_wrw_plan", &conv3x3p1_wrw_plan,
        "(m-blocks, rows per pass, resident blocks) of a conv3x3p1_wrw call",
        py::arg("N"), py::arg("H"), py::arg("W"), py::arg("C"),
        py::arg("COUT"), py::arg("any_hw") = false);
  m.def("conv3x3c4_wrw_plan", &conv3x3c4_wrw_plan,
        "(m-blocks, rows per pass, resident blocks) of a stem wrw call",
        py::arg("N"), py::arg("H"), py::arg("W"), py::arg("hw"));
  m.def("maxpool3x3s2_fwd", &maxpool3x3s2_fwd,
        "NHWC bf16 max-pool 3x3 s2 pad-1 fwd; uint8 tap plane, or none when "
        "idx is empty");
  m.def("maxpool3x3s2_bwd", &maxpool3x3s2_bwd,
        "max-pool 3x3 s2 pad-1 input-grad: ordered gather over the tap "
        "plane, every gx element written once");
  m.def("maxpool3x3s2_supported", &maxpool3x3s2_supported);
}
