// FreeU (Si et al., "FreeU: Free Lunch in Diffusion U-Net") at the decoder's concatenations, for gfx950 — sampling only, opt-in.
//
// The call site is the hand-over of the (hidden, skip) pair to an up block's ResBlock (e4t/models/unet_2d_blocks.py, CrossAttnUpBlock2D /
// UpBlock2D.forward_nhwc).  Operands are NHWC matrices: h [B*HW][C_h], k [B*HW][C_k], bf16.  Two launches per marked ResBlock:
//   e4t_freeu_stats   skip:   the seven real numbers of X[0,0], X[-1,0], X[0,-1], X[-1,-1] per (image, skip channel) — with FreeU's threshold
//                             of 1 the Fourier filter touches no other frequency, so the fftn / ifftn pair of the usual recipe is this column
//                             reduction and one elementwise pass
//                     hidden: (version 2) the per-pixel channel SUM and its minimum / maximum over every 1/64 of an image's rows.  m^ =
//                             (m - min) / (max - min) does not change under the mean's 1 / C_h, and the sum needs no rounding the mean
//                             would add: where one value dominates (the bf16 inputs then share an exponent) the sums are exact, while a
//                             mean rounded to fp32 would already cost m^ 2e-5 at C_h = 1280.  The 64 (min, max) pairs per image are
//                             folded by the apply kernel with one wave-wide load: min / max are exact in any order, so no workgroup of
//                             the statistics launch waits for another
//   e4t_freeu_apply   h' = h * ((b - 1) m^ + 1) on the first C_h / 2 channels (version 1: h' = b h), k' = k + (s - 1) LP(k)
//
// How the column reduction is split (the one real choice): ONE workgroup owns a slab of 32 skip channels of one image and walks all HW rows,
// so every coefficient is written once by one workgroup — no partials across workgroups, no second pass, no atomics.  Inside the workgroup a
// row is read as 4 lanes x 16 bytes (one 64-byte segment) by 64 row lanes (16 per wave); a lane walks its rows in ascending order with four
// loads in flight, the 16 row lanes of a wave are folded by an xor butterfly and the 4 waves in wave order through LDS: a fixed order, so
// eager and replayed runs agree to the bit.  That is B * C_k / 32 workgroups (20 at 64x64x320, B = 2; 80 at 8x8x1280), and the walk is bound
// by latency inside the workgroup (every lane's rows are a serial walk), not by memory bandwidth (654 GB/s at the first of these shapes).  Narrower slabs were measured (8 or 16 channels whenever
// that still left fewer than 128 workgroups): 64x64x320 went from 23.3 to 20.8 us, but 8x8x1280, 16x16x640 and 32x32x320 from 10.5 / 10.5 /
// 12.8 to 12.1 / 14.1 / 14.4 us (a lane then reads 16 bytes of a 128-byte line 256 rows apart, and every workgroup pays its own phase table
// and fold), so the slab stayed at 32 channels.  The phases 2 pi y / H and 2 pi x / W take H + W values: their sines and cosines are
// evaluated once per workgroup in double precision (sincospi: exact at the quadrant points) into LDS and rounded once to fp32.
#include "common.h"
#include "../../include/e4t_hip.h"
#include <math.h>

namespace {

constexpr int FREEU_THREADS = 256;
constexpr int FREEU_SLAB_VECS = 4;        // 16-byte vectors (8 channels each) per coefficient workgroup: a 32-channel slab, 64 row lanes
constexpr int FREEU_UNROLL = 4;           // rows a lane of a coefficient workgroup has in flight
constexpr int FREEU_COEFS = E4T_FREEU_COEFS;
constexpr int FREEU_MM = E4T_FREEU_MM_CHUNKS;
constexpr int FREEU_MAX_PHASES = 4096;    // H + W: 32 KiB of LDS for the sine / cosine tables
constexpr int FREEU_APPLY_VECS = 16;      // e4t_freeu_apply: a workgroup is 16 vectors (256 bytes of a row) x 16 row lanes ...
constexpr int FREEU_APPLY_ROWS = 256;     // ... walking 256 rows, so the 7 x 8 coefficients a lane holds serve 16 rows

struct FreeuDims {
  int B, H, W, HW, Ch, Ck;
};
// offsets (in floats) of the workspace's fields
struct FreeuLayout {
  size_t coef, msum, mm, total;
};
__host__ __device__ inline FreeuLayout freeu_layout(int B, int HW, int Ck) {
  FreeuLayout L;
  L.coef = 0;                                          // [B][7][C_k]
  L.msum = L.coef + (size_t)B * FREEU_COEFS * Ck;      // [B][HW]: sum of the pixel's C_h channels
  L.mm = L.msum + (size_t)B * HW;                      // [B][64][2]: (min, max) of the sums of 1/64 of the rows
  L.total = L.mm + (size_t)B * FREEU_MM * 2;
  return L;
}

// cos / sin of 2 pi i / H (i < H) and 2 pi (i - H) / W (H <= i < H + W) -> tc / ts [H + W]
__device__ __forceinline__ void fill_phases(int H, int W, float* tc, float* ts) {
  for (int i = threadIdx.x; i < H + W; i += FREEU_THREADS) {
    const double a = i < H ? 2.0 * (double)i / (double)H : 2.0 * (double)(i - H) / (double)W;
    double sn, cs;
    sincospi(a, &sn, &cs);
    tc[i] = (float)cs;
    ts[i] = (float)sn;
  }
}

// the six non-constant basis functions of a pixel: cos / sin of theta_y, phi_x and theta_y + phi_x
__device__ __forceinline__ void basis(const float* tc, const float* ts, int H, int W, int p, float* bs) {
  const int y = p / W, x = p - y * W;
  const float cy = tc[y], sy = ts[y], cx = tc[H + x], sx = ts[H + x];
  bs[0] = cy; bs[1] = sy; bs[2] = cx; bs[3] = sx;
  bs[4] = fmaf(cy, cx, -sy * sx);
  bs[5] = fmaf(sy, cx, cy * sx);
}

__global__ __launch_bounds__(FREEU_THREADS) void freeu_stats_kernel(const bf16_t* __restrict__ h, int ldh, const bf16_t* __restrict__ k, int ldk,
                                                                    float* __restrict__ ws, FreeuDims dm, int nslab, int ncoef_wg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int SV = FREEU_SLAB_VECS, ROW_LANES = FREEU_THREADS / SV;
  __shared__ float red[4 * SV * FREEU_COEFS * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = dm.HW;
  const FreeuLayout L = freeu_layout(dm.B, HW, dm.Ck);
  if ((int)blockIdx.x < ncoef_wg) {
    // ---- skip: X[0,0], X[-1,0], X[0,-1], X[-1,-1] of a 32-channel slab of one image --------------------------------------------------
    const int b = blockIdx.x / nslab, slab = blockIdx.x - b * nslab;
    float* tc = (float*)smem;
    float* ts = tc + dm.H + dm.W;
    fill_phases(dm.H, dm.W, tc, ts);
    __syncthreads();
    const int cv = lane & (SV - 1);
    const int rg = lane / SV + (64 / SV) * wave;
    const int c0 = (slab * SV + cv) * 8;
    const bool live = c0 < dm.Ck;                       // (C_k % 8 == 0: a vector is inside or outside as a whole)
    float acc[FREEU_COEFS][8];
#pragma unroll
    for (int j = 0; j < FREEU_COEFS; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[j][e] = 0.f;
    if (live) {
      const bf16_t* kp = k + (size_t)b * HW * ldk + c0;
      for (int p = rg; p < HW; p += FREEU_UNROLL * ROW_LANES) {
        // the lane's next four rows are loaded before the first is used: the walk is a chain of dependent loads otherwise (64 round
        // trips at 64 x 64); they are accumulated in ascending row order, and a row past the end adds zeros
        uint4 q[FREEU_UNROLL];
#pragma unroll
        for (int u = 0; u < FREEU_UNROLL; ++u) {
          const int pu = p + u * ROW_LANES;
          q[u] = pu < HW ? *(const uint4*)(kp + (size_t)pu * ldk) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < FREEU_UNROLL; ++u) {
          float f[8], bs[6];
          unpack8(q[u], f);
          basis(tc, ts, dm.H, dm.W, min(p + u * ROW_LANES, HW - 1), bs);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            acc[0][e] += f[e];
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[j + 1][e] = fmaf(f[e], bs[j], acc[j + 1][e]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FREEU_COEFS; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v = acc[j][e];
#pragma unroll
        for (int o = SV; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        if (lane < SV) red[((wave * SV + cv) * FREEU_COEFS + j) * 8 + e] = v;
      }
    __syncthreads();
    if (tid < SV * FREEU_COEFS * 8) {
      const int v = tid / (FREEU_COEFS * 8), j = (tid / 8) % FREEU_COEFS, e = tid & 7;
      const int c = (slab * SV + v) * 8 + e;
      if (c < dm.Ck) {
        float t = red[tid];
        for (int w = 1; w < 4; ++w) t += red[w * SV * FREEU_COEFS * 8 + tid];
        ws[L.coef + ((size_t)b * FREEU_COEFS + j) * dm.Ck + c] = t;
      }
    }
    return;
  }
  // ---- hidden (version 2): channel sum of every pixel, one wave per row; min / max of this 1/64 of the image's rows ------------------
  const int idx = blockIdx.x - ncoef_wg;
  const int b = idx / FREEU_MM, chunk = idx - b * FREEU_MM;
  const int per = (HW + FREEU_MM - 1) / FREEU_MM;
  const int p0 = min(chunk * per, HW), p1 = min(p0 + per, HW);
  float mn = INFINITY, mx = -INFINITY;
  for (int p = p0 + wave; p < p1; p += 4) {
    const bf16_t* hp = h + ((size_t)b * HW + p) * ldh;
    float s = 0.f;
    for (int c = lane * 8; c < dm.Ch; c += 64 * 8) {
      float f[8];
      unpack8(*(const uint4*)(hp + c), f);
      s += ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
    }
    const float m = wave_sum(s);
    if (lane == 0) ws[L.msum + (size_t)b * HW + p] = m;
    mn = fminf(mn, m);
    mx = fmaxf(mx, m);
  }
  if (lane == 0) { red[wave] = mn; red[4 + wave] = mx; }
  __syncthreads();
  if (tid == 0) {                                       // a chunk without rows leaves (+inf, -inf): neutral in the apply kernel's fold
    float* o = ws + L.mm + ((size_t)b * FREEU_MM + chunk) * 2;
    o[0] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
    o[1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  }
}

// grid (vector blocks, row blocks, B); thread = one 16-byte vector of the concatenated row [h | k], walking its workgroup's rows 16 apart
__global__ __launch_bounds__(FREEU_THREADS) void freeu_apply_kernel(const bf16_t* __restrict__ h, int ldh, const bf16_t* __restrict__ k, int ldk,
                                                                    const float* __restrict__ ws, bf16_t* __restrict__ ho, int ldho,
                                                                    bf16_t* __restrict__ ko, int ldko, FreeuDims dm, float bb, float ss, int version) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ float mmv[2];
  float* tc = (float*)smem;
  float* ts = tc + dm.H + dm.W;
  const int tid = threadIdx.x, b = blockIdx.z, HW = dm.HW;
  const float bm1 = bb - 1.f, sm1 = ss - 1.f;
  const FreeuLayout L = freeu_layout(dm.B, HW, dm.Ck);
  fill_phases(dm.H, dm.W, tc, ts);
  if (version == 2 && tid < 64) {                       // wave 0 folds the image's 64 (min, max) pairs: exact, whatever the order
    const float* mm = ws + L.mm + ((size_t)b * FREEU_MM + tid) * 2;
    float mn = mm[0], mx = mm[1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o, 64));
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    if (tid == 0) { mmv[0] = mn; mmv[1] = mx; }
  }
  __syncthreads();
  const int nvh = dm.Ch >> 3, nvk = dm.Ck >> 3;
  const int v = blockIdx.x * FREEU_APPLY_VECS + (tid & (FREEU_APPLY_VECS - 1));
  if (v >= nvh + nvk) return;
  const int r0 = blockIdx.y * FREEU_APPLY_ROWS + (tid >> 4);
  const int r1 = min((int)(blockIdx.y + 1) * FREEU_APPLY_ROWS, HW);
  if (v < nvh) {
    const bf16_t* hp = h + (size_t)b * HW * ldh + v * 8;
    bf16_t* op = ho + (size_t)b * HW * ldho + v * 8;
    const bool scaled = v < (nvh >> 1);                 // the first C_h / 2 channels (C_h % 16 == 0: whole vectors)
    const float mn = version == 2 ? mmv[0] : 0.f, mx = version == 2 ? mmv[1] : 0.f;
    const float range = mx - mn;
    const float* msum = ws + L.msum + (size_t)b * HW;
    for (int p = r0; p < r1; p += 16) {
      const uint4 q = *(const uint4*)(hp + (size_t)p * ldh);
      if (!scaled) {
        *(uint4*)(op + (size_t)p * ldho) = q;
        continue;
      }
      float sc = bb;                                    // version 1
      if (version == 2) {
        const float mh = range > 0.f ? (msum[p] - mn) / range : 0.f;
        sc = fmaf(bm1, mh, 1.f);
      }
      float f[8];
      unpack8(q, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] *= sc;
      *(uint4*)(op + (size_t)p * ldho) = pack8(f);
    }
    return;
  }
  const int c0 = (v - nvh) * 8;
  const bf16_t* kp = k + (size_t)b * HW * ldk + c0;
  bf16_t* op = ko + (size_t)b * HW * ldko + c0;
  float cf[FREEU_COEFS][8];
  const float invhw = 1.f / (float)HW;
#pragma unroll
  for (int j = 0; j < FREEU_COEFS; ++j) {
    const float4* cp = (const float4*)(ws + L.coef + ((size_t)b * FREEU_COEFS + j) * dm.Ck + c0);
    const float4 a = cp[0], c = cp[1];
    cf[j][0] = a.x * invhw; cf[j][1] = a.y * invhw; cf[j][2] = a.z * invhw; cf[j][3] = a.w * invhw;
    cf[j][4] = c.x * invhw; cf[j][5] = c.y * invhw; cf[j][6] = c.z * invhw; cf[j][7] = c.w * invhw;
  }
  for (int p = r0; p < r1; p += 16) {
    float f[8], bs[6];
    unpack8(*(const uint4*)(kp + (size_t)p * ldk), f);
    basis(tc, ts, dm.H, dm.W, p, bs);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float lp = cf[0][e];
#pragma unroll
      for (int j = 0; j < 6; ++j) lp = fmaf(cf[j + 1][e], bs[j], lp);
      f[e] = fmaf(sm1, lp, f[e]);                       // s = 1: k + 0 * lp = k, bit for bit
    }
    *(uint4*)(op + (size_t)p * ldko) = pack8(f);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check_dims(const char* what, int B, int H, int W, int Ch, int Ck, int version, FreeuDims* dm) {
  E4T_REQUIRE(B >= 1 && B <= 65535, "%s: B=%d outside [1, 65535]", what, B);
  E4T_REQUIRE(H >= 2 && W >= 2, "%s: map %dx%d (both sides must be >= 2)", what, H, W);
  E4T_REQUIRE(H + W <= FREEU_MAX_PHASES, "%s: H + W = %d exceeds %d", what, H + W, FREEU_MAX_PHASES);
  E4T_REQUIRE(Ch >= 16 && Ch % 16 == 0, "%s: C_h=%d must be a positive multiple of 16", what, Ch);
  E4T_REQUIRE(Ck >= 8 && Ck % 8 == 0, "%s: C_k=%d must be a positive multiple of 8", what, Ck);
  E4T_REQUIRE(version == 1 || version == 2, "%s: version=%d (1 or 2)", what, version);
  E4T_REQUIRE((long long)B * H * W <= 0x7fffffffLL, "%s: B=%d %dx%d is too large", what, B, H, W);
  *dm = FreeuDims{B, H, W, H * W, Ch, Ck};
  return 0;
}

}  // namespace

extern "C" int e4t_freeu_stats(const void* h, int ldh, const void* k, int ldk, float* ws, int B, int H, int W, int Ch, int Ck, int version,
                               e4t_stream stream) {
  E4T_REQUIRE(h && k && ws, "freeu_stats: null operand");
  FreeuDims dm;
  if (int rc = check_dims("freeu_stats", B, H, W, Ch, Ck, version, &dm)) return rc;
  E4T_REQUIRE(ldh >= Ch && ldk >= Ck && ldh % 8 == 0 && ldk % 8 == 0 && aligned16(h) && aligned16(k) && aligned16(ws),
              "freeu_stats: rows must be 16-byte aligned (ldh=%d ldk=%d)", ldh, ldk);
  const int nslab = cdiv(Ck, FREEU_SLAB_VECS * 8);
  const int ncoef = B * nslab, nmean = version == 2 ? B * FREEU_MM : 0;
  const size_t lds = (size_t)2 * (H + W) * sizeof(float);
  hipLaunchKernelGGL(freeu_stats_kernel, dim3(ncoef + nmean), dim3(FREEU_THREADS), lds, (hipStream_t)stream, (const bf16_t*)h, ldh, (const bf16_t*)k,
                     ldk, ws, dm, nslab, ncoef);
  E4T_CHECK_LAUNCH("freeu_stats_kernel");
  E4T_LOG_LAUNCH("freeu_stats_kernel|B%d %dx%d Ch%d Ck%d v%d|%.0f|%.0f", B, H, W, Ch, Ck, version,
                 2.0 * B * dm.HW * (double)(Ck + (version == 2 ? Ch : 0)), 14.0 * B * dm.HW * (double)Ck);
  return 0;
}

extern "C" int e4t_freeu_apply(const void* h, int ldh, const void* k, int ldk, const float* ws, void* h_out, int ldho, void* k_out, int ldko, int B,
                               int H, int W, int Ch, int Ck, float b, float s, int version, e4t_stream stream) {
  E4T_REQUIRE(h && k && ws && h_out && k_out, "freeu_apply: null operand");
  FreeuDims dm;
  if (int rc = check_dims("freeu_apply", B, H, W, Ch, Ck, version, &dm)) return rc;
  E4T_REQUIRE(ldh >= Ch && ldk >= Ck && ldho >= Ch && ldko >= Ck && ldh % 8 == 0 && ldk % 8 == 0 && ldho % 8 == 0 && ldko % 8 == 0 && aligned16(h) &&
                  aligned16(k) && aligned16(ws) && aligned16(h_out) && aligned16(k_out),
              "freeu_apply: rows must be 16-byte aligned (ldh=%d ldk=%d ldho=%d ldko=%d)", ldh, ldk, ldho, ldko);
  E4T_REQUIRE(h_out != h && k_out != k, "freeu_apply: the outputs are new buffers (the statistics describe the inputs)");
  const dim3 grid(cdiv((Ch + Ck) / 8, FREEU_APPLY_VECS), cdiv(dm.HW, FREEU_APPLY_ROWS), B);
  const size_t lds = (size_t)2 * (H + W) * sizeof(float);
  hipLaunchKernelGGL(freeu_apply_kernel, grid, dim3(FREEU_THREADS), lds, (hipStream_t)stream, (const bf16_t*)h, ldh, (const bf16_t*)k, ldk, ws,
                     (bf16_t*)h_out, ldho, (bf16_t*)k_out, ldko, dm, b, s, version);
  E4T_CHECK_LAUNCH("freeu_apply_kernel");
  E4T_LOG_LAUNCH("freeu_apply_kernel|B%d %dx%d Ch%d Ck%d v%d|%.0f|%.0f", B, H, W, Ch, Ck, version, 4.0 * B * dm.HW * (double)(Ch + Ck),
                 14.0 * B * dm.HW * (double)Ck);
  return 0;
}
