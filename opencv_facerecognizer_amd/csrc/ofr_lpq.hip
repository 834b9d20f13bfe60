// OriginalLBP and LPQ codes and per-cell histograms on gfx950.
//
// Replaces OriginalLBP.__call__ (reference lbp.py:55-72) and LPQ.__call__ (lbp.py:211-318) under
// SpatialHistogram.spatially_enhanced_histogram (feature.py:286-302).  Both descriptors give 8-bit
// codes, all inside the histogram range, so a cell's float histogram is count / (py * px) exactly.
//
// OriginalLBP: integer compares of the 3x3 ring against the centre (bit 7..0 = NW, N, NE, E, SE, S,
// SW, W), bit-exact.  Memory-bound: a thread loads the aligned dwords that cover 6 bytes of each of
// three image rows, aligns them in registers and produces 4 horizontally adjacent codes.
//
// LPQ: four separable complex responses of a (2r+1)^2 window, decorrelated by an 8x8 matrix from
// the host, sign-quantised.  A workgroup owns strips of image rows: the strip and its r-row halo
// are staged in LDS as bytes; a column pass leaves three fp64 planes per strip in LDS (the w0 sum and
// the complex w1 sum over rows), zero-bordered by r columns so the row pass needs no bounds test; the
// row pass reads its n taps from them at unit lane stride (adjacent lanes = adjacent pixels, no bank
// conflicts), forms Qa..Qd (Qc and Qd share their four product sums), applies V^T and packs the
// eight signs in registers.  Taps and V are kernel arguments (scalar loads).  The code of pixel (r, c) belongs at
// linear index c*H + r of the [H][W] output (the reference flattens column-major and reshapes
// row-major); the fused form counts it straight into LDS counters of the whole grid.
// The kernel is typed on the pixel: float32 / float64 images (ofr_lpq_codes_f / ofr_lpq_hist_f) stage the
// strip in their own width and run the same fp64 formulation.  (OriginalLBP on float images: ofr_lbp_float.hip.)
#include <cmath>

#include "ofr_common.h"

namespace ofr {
namespace lpq {

constexpr int MAXR = 8;
constexpr int THREADS = 1024;
constexpr int PX = 2;  // pixels a thread carries per step
constexpr int LDS_BUDGET = 160 * 1024;
constexpr int MAX_STRIP = 32;
constexpr int64_t MAX_PIXELS = 1 << 22;  // fdiv's range

enum { MODE_CODES = 0, MODE_HIST_LDS = 1, MODE_HIST_GLOBAL = 2 };

struct Args {
  int H, W, gr, gc, py, px;
  int SR;             // image rows per strip
  int strips_per_wg;  // strips one workgroup walks
  int mode;
  int count_bytes;
  int atomic_flush;   // several workgroups per image: counters are added to a zeroed destination
  float inv_W, inv_py, inv_px;
  int R;
  double tap[2 * MAXR + 1][2];  // (Re, Im) of w1(u) = exp(-2 pi i u / n), u = -r..r
  double Vt[8][8];              // V transposed: G_k = sum_j Vt[k][j] F_j
};

// a / d for 0 <= a < 2^22, inv = 1.0f / d: the fp32 product is within 1/2 of the quotient
__device__ __forceinline__ int fdiv(int a, int d, float inv) {
  int q = (int)((float)a * inv);
  const int r = a - q * d;
  if (r < 0) --q;
  else if (r >= d) ++q;
  return q;
}

// counter `idx` of an image's packed destination: the word that holds it and its unit there
__device__ __forceinline__ void count_global(uint32_t* dst, int idx, int count_bytes) {
  if (count_bytes == 1) atomicAdd(dst + (idx >> 2), 1u << (8 * (idx & 3)));
  else if (count_bytes == 2) atomicAdd(dst + (idx >> 1), 1u << (16 * (idx & 1)));
  else atomicAdd(dst + idx, 1u);
}

// LDS counters [total] -> packed 1/2/4-byte counts; `atomic`: add the non-zero words instead (no
// byte or half ever carries: every partial sum is at most the cell's pixel count)
__device__ __forceinline__ void flush_counts(const uint32_t* hist, int total, uint32_t* o, int count_bytes,
                                             bool atomic) {
  const int per = 4 / count_bytes;
  for (int i = threadIdx.x; i < total / per; i += blockDim.x) {
    uint32_t w;
    if (count_bytes == 1) w = hist[4 * i] | (hist[4 * i + 1] << 8) | (hist[4 * i + 2] << 16) | (hist[4 * i + 3] << 24);
    else if (count_bytes == 2) w = hist[2 * i] | (hist[2 * i + 1] << 16);
    else w = hist[i];
    if (!atomic) o[i] = w;
    else if (w) atomicAdd(o + i, w);
  }
}

__global__ void __launch_bounds__(256) zero_kernel(uint32_t* __restrict__ p, int64_t nwords) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
}

// T: the pixel type.  uint8_t is the byte path; float / double (ofr_lpq_*_f) stage the strip in their own
// width -- the tile is copied as dwords either way -- and sum the w0 response in fp64 instead of uint32.
template <typename T>
__global__ void __launch_bounds__(THREADS) lpq_kernel(const T* __restrict__ imgs, Args a, void* __restrict__ out) {
  constexpr bool BYTES = sizeof(T) == 1;
  const int R = a.R, N = 2 * R + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int H = a.H, W = a.W, Wp = W + 2 * R, SR = a.SR;
  const int ncnt = a.mode == MODE_HIST_LDS ? a.gr * a.gc * 256 : 0;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
  double* pl0 = reinterpret_cast<double*>(smem + (size_t)ncnt * 4);  // w0 sums   [SR][Wp]
  double* plr = pl0 + SR * Wp;                                       // Re w1 sums
  double* pli = plr + SR * Wp;                                       // Im w1 sums
  T* tile = reinterpret_cast<T*>(pli + SR * Wp);                     // [SR + 2R][W] pixels
  const int64_t img = blockIdx.y;
  const int64_t npix = (int64_t)H * W;
  const T* im = imgs + img * npix;
  const int ncell = a.gr * a.gc;
  uint32_t* gcounts = reinterpret_cast<uint32_t*>((uint8_t*)out + img * (int64_t)ncell * 256 * a.count_bytes);

  for (int i = threadIdx.x; i < ncnt; i += THREADS) hist[i] = 0;
  for (int i = threadIdx.x; i < 3 * SR * Wp; i += THREADS) pl0[i] = 0.0;  // the r-column borders stay zero

  const int nstrips = (H + SR - 1) / SR;
  const int s0 = blockIdx.x * a.strips_per_wg, s1 = min(nstrips, s0 + a.strips_per_wg);
  const bool dwords = ((W * (int)sizeof(T)) & 3) == 0 && ((uintptr_t)im & 3) == 0;
  const uint8_t* imb = reinterpret_cast<const uint8_t*>(im);
  const int64_t nbytes = npix * (int64_t)sizeof(T);
  for (int s = s0; s < s1; ++s) {
    const int y0 = s * SR, rows = min(SR, H - y0);
    __syncthreads();  // the previous strip's row pass is done with the planes
    // tile row t = image row y0 - R + t; rows are contiguous, so one flat copy, zero outside the image
    const int tbytes = (rows + 2 * R) * W * (int)sizeof(T);
    const int64_t off0 = (int64_t)(y0 - R) * W * (int64_t)sizeof(T);
    if (dwords) {
      for (int i = threadIdx.x; i < tbytes / 4; i += THREADS) {
        const int64_t off = off0 + 4 * (int64_t)i;
        reinterpret_cast<uint32_t*>(tile)[i] = (off >= 0 && off < nbytes) ? *reinterpret_cast<const uint32_t*>(imb + off) : 0u;
      }
    } else {
      for (int i = threadIdx.x; i < tbytes; i += THREADS) {
        const int64_t off = off0 + i;
        reinterpret_cast<uint8_t*>(tile)[i] = (off >= 0 && off < nbytes) ? imb[off] : (uint8_t)0;
      }
    }
    __syncthreads();
    // column pass: S(y, x) = sum_u w(u) X(y - u, x); tile row of image row y - u is yy + 2R - k, k = u + R
    // A thread takes PX pixels THREADS apart per step (each wave still covers adjacent pixels).  The tap
    // loops stay rolled: a tap, or a row of V^T, is a scalar load from the kernel arguments that serves
    // PX pixels, and the planes' values are in flight for one tap pair only, not for the whole window.
    const int npx = rows * W;
    for (int i0 = threadIdx.x; i0 < npx; i0 += THREADS * PX) {
      const T* col[PX];
      int o[PX];
      uint32_t sum[PX];   // w0 response of bytes: exact in integers
      double sumd[PX];    // ... of float pixels
      double sr[PX], si[PX];
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int i = min(i0 + p * THREADS, npx - 1);
        const int yy = fdiv(i, W, a.inv_W), x = i - yy * W;
        col[p] = tile + (yy + 2 * R) * W + x;
        o[p] = yy * Wp + x + R;
        sum[p] = 0;
        sumd[p] = sr[p] = si[p] = 0.0;
      }
#pragma unroll 2
      for (int k = 0; k < N; ++k) {
        const double tr = a.tap[k][0], ti = a.tap[k][1];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
          const T b = col[p][-k * W];
          const double v = (double)b;
          if constexpr (BYTES) sum[p] += b;
          else sumd[p] += v;
          sr[p] += tr * v;
          si[p] += ti * v;
        }
      }
#pragma unroll
      for (int p = 0; p < PX; ++p) {  // a clamped duplicate rewrites the last pixel's own values
        pl0[o[p]] = BYTES ? (double)sum[p] : sumd[p];
        plr[o[p]] = sr[p];
        pli[o[p]] = si[p];
      }
    }
    __syncthreads();
    // row pass: Q(y, x) = sum_v b(v) S(y, x - v); plane column of x - v is x + 2R - k, k = v + R
    for (int i0 = threadIdx.x; i0 < npx; i0 += THREADS * PX) {
      int base[PX], pos[PX];
      double acc[PX][8];
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int i = min(i0 + p * THREADS, npx - 1);
        const int yy = fdiv(i, W, a.inv_W), x = i - yy * W;
        base[p] = yy * Wp + x + 2 * R;
        pos[p] = x * H + y0 + yy;  // column-major flatten, row-major reshape
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = 0.0;
      }
#pragma unroll 2
      for (int k = 0; k < N; ++k) {
        const double tr = a.tap[k][0], ti = a.tap[k][1];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
          const double z0 = pl0[base[p] - k], zr = plr[base[p] - k], zi = pli[base[p] - k];
          acc[p][0] += tr * z0;  // Qa = w0 (rows) x w1 (columns)
          acc[p][1] += ti * z0;
          acc[p][2] += zr;        // Qb = w1 x w0
          acc[p][3] += zi;
          acc[p][4] += tr * zr;  // A;  Qc = w1 x w1 = (A - B) + i (C + D)
          acc[p][5] += ti * zi;  // B;  Qd = w1 x w2 = (A + B) + i (C - D)
          acc[p][6] += tr * zi;  // C
          acc[p][7] += ti * zr;  // D
        }
      }
      uint32_t code[PX];
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const double A = acc[p][4], B = acc[p][5], C = acc[p][6], D = acc[p][7];
        acc[p][4] = A - B;
        acc[p][5] = C + D;
        acc[p][6] = A + B;
        acc[p][7] = C - D;
        code[p] = 0;
      }
#pragma unroll 1
      for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int p = 0; p < PX; ++p) {
          double g = a.Vt[k][0] * acc[p][0];
#pragma unroll
          for (int j = 1; j < 8; ++j) g += a.Vt[k][j] * acc[p][j];
          code[p] |= (g >= 0.0 ? 1u : 0u) << k;
        }
      }
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        if (i0 + p * THREADS >= npx) continue;
        if (a.mode == MODE_CODES) {
          reinterpret_cast<uint8_t*>(out)[img * npix + pos[p]] = (uint8_t)code[p];
        } else {
          const int orow = fdiv(pos[p], W, a.inv_W), ocol = pos[p] - orow * W;
          if (orow < a.gr * a.py && ocol < a.gc * a.px) {
            const int idx = (fdiv(orow, a.py, a.inv_py) * a.gc + fdiv(ocol, a.px, a.inv_px)) * 256 + (int)code[p];
            if (a.mode == MODE_HIST_LDS) atomicAdd(&hist[idx], 1u);
            else count_global(gcounts, idx, a.count_bytes);
          }
        }
      }
    }
  }
  if (a.mode == MODE_HIST_LDS) {
    __syncthreads();
    flush_counts(hist, ncell * 256, gcounts, a.count_bytes, a.atomic_flush != 0);
  }
}

// ---- OriginalLBP ------------------------------------------------------------------------------
// bytes p[0 .. nbytes) (3 <= nbytes <= 6) in the low bytes of the result, from the aligned dwords
// that hold at least one of them
__device__ __forceinline__ uint64_t load_bytes(const uint8_t* p, int nbytes) {
  const int sh = (int)((uintptr_t)p & 3);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p - sh);
  const uint32_t d0 = w[0];
  const uint32_t d1 = 4 - sh < nbytes ? w[1] : 0u;
  const uint32_t d2 = 8 - sh < nbytes ? w[2] : 0u;
  const uint64_t lo = ((uint64_t)d1 << 32) | d0;
  return (lo >> (8 * sh)) | (sh ? ((uint64_t)d2 << (64 - 8 * sh)) : 0ull);
}

__device__ __forceinline__ uint32_t byte_of(uint64_t v, int k) { return (uint32_t)(v >> (8 * k)) & 0xffu; }

// code j (0..3) of the 6-byte windows r0 (above), r1, r2 (below)
__device__ __forceinline__ uint32_t olbp_code(uint64_t r0, uint64_t r1, uint64_t r2, int j) {
  const uint32_t c = byte_of(r1, j + 1);
  return ((byte_of(r0, j) >= c ? 1u : 0u) << 7) | ((byte_of(r0, j + 1) >= c ? 1u : 0u) << 6) |
         ((byte_of(r0, j + 2) >= c ? 1u : 0u) << 5) | ((byte_of(r1, j + 2) >= c ? 1u : 0u) << 4) |
         ((byte_of(r2, j + 2) >= c ? 1u : 0u) << 3) | ((byte_of(r2, j + 1) >= c ? 1u : 0u) << 2) |
         ((byte_of(r2, j) >= c ? 1u : 0u) << 1) | (byte_of(r1, j) >= c ? 1u : 0u);
}

struct OlbpArgs {
  int H, W, dy, dx;  // image and code-image sizes
  int gr, gc, py, px;
  int rows_per_wg;   // cell rows per workgroup
  int count_bytes;
};

__global__ void __launch_bounds__(256) olbp_codes_kernel(const uint8_t* __restrict__ imgs, OlbpArgs a,
                                                         uint8_t* __restrict__ codes) {
  const int64_t img = blockIdx.y;
  const uint8_t* im = imgs + img * (int64_t)a.H * a.W;
  uint8_t* out = codes + img * (int64_t)a.dy * a.dx;
  const int ng = (a.dx + 3) >> 2;  // groups of 4 codes per row
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < a.dy * ng; i += gridDim.x * blockDim.x) {
    const int y = i / ng, x0 = 4 * (i - y * ng);
    const int cnt = min(4, a.dx - x0);
    const uint8_t* p = im + (int64_t)y * a.W + x0;
    const uint64_t r0 = load_bytes(p, cnt + 2), r1 = load_bytes(p + a.W, cnt + 2), r2 = load_bytes(p + 2 * a.W, cnt + 2);
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) packed |= olbp_code(r0, r1, r2, j) << (8 * j);
    uint8_t* o = out + (int64_t)y * a.dx + x0;
    if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
      *reinterpret_cast<uint32_t*>(o) = packed;
    } else {
      for (int j = 0; j < cnt; ++j) o[j] = (uint8_t)(packed >> (8 * j));
    }
  }
}

// one workgroup per (image, band of cell rows), u32 LDS counters of the band, plain packed stores
__global__ void __launch_bounds__(512) olbp_hist_kernel(const uint8_t* __restrict__ imgs, OlbpArgs a,
                                                        void* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const int64_t img = blockIdx.y;
  const int cr0 = blockIdx.x * a.rows_per_wg, cr1 = min(a.gr, cr0 + a.rows_per_wg);
  const int total = (cr1 - cr0) * a.gc * 256;
  for (int i = threadIdx.x; i < total; i += blockDim.x) hist[i] = 0;
  __syncthreads();
  const uint8_t* im = imgs + img * (int64_t)a.H * a.W;
  const int wpx = a.gc * a.px;  // covered code columns
  const int ng = (wpx + 3) >> 2;
  const int nrows = (cr1 - cr0) * a.py;
  for (int i = threadIdx.x; i < nrows * ng; i += blockDim.x) {
    const int yy = i / ng, x0 = 4 * (i - yy * ng);
    const int cnt = min(4, wpx - x0);
    const uint8_t* p = im + (int64_t)(cr0 * a.py + yy) * a.W + x0;
    const uint64_t r0 = load_bytes(p, cnt + 2), r1 = load_bytes(p + a.W, cnt + 2), r2 = load_bytes(p + 2 * a.W, cnt + 2);
    const int crow = (yy / a.py) * a.gc;
    int cx = x0 / a.px, rx = x0 - cx * a.px;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) atomicAdd(&hist[(crow + cx) * 256 + (int)olbp_code(r0, r1, r2, j)], 1u);
      if (++rx == a.px) {
        rx = 0;
        ++cx;
      }
    }
  }
  __syncthreads();
  const int64_t cell_base = img * (int64_t)a.gr * a.gc + (int64_t)cr0 * a.gc;
  flush_counts(hist, total, reinterpret_cast<uint32_t*>((uint8_t*)counts + cell_base * 256 * a.count_bytes),
               a.count_bytes, false);
}

// ---- host side ----------------------------------------------------------------------------------
static int check_grid(const char* who, int dy, int dx, int gr, int gc, const void* counts, int count_bytes, int& py,
                      int& px) {
  const std::string w(who);
  if (gr < 1 || gc < 1) return fail(OFR_E_INVALID, w + ": bad grid");
  if (count_bytes != 1 && count_bytes != 2 && count_bytes != 4)
    return fail(OFR_E_INVALID, w + ": count_bytes must be 1, 2 or 4");
  if (gr > dy || gc > dx) return fail(OFR_E_INVALID, w + ": grid larger than the code image");
  py = dy / gr;
  px = dx / gc;
  const int64_t cell = (int64_t)py * px;
  if ((count_bytes == 1 && cell > 255) || (count_bytes == 2 && cell > 65535))
    return fail(OFR_E_INVALID, w + ": cell too large for count_bytes");
  if ((uintptr_t)counts & 3) return fail(OFR_E_INVALID, w + ": counts must be 4-byte aligned");
  return OFR_OK;
}

template <typename T>
static int launch(hipStream_t st, const T* imgs, int64_t n, const Args& a, void* out, size_t lds,
                  size_t img_out_bytes) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)lpq_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BUDGET);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(lpq_kernel)");
    attr = true;
  }
  const int nstrips = (int)cdiv(a.H, a.SR);
  const unsigned gx = (unsigned)cdiv(nstrips, a.strips_per_wg);
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    hipLaunchKernelGGL(lpq_kernel<T>, dim3(gx, (unsigned)chunk), dim3(THREADS), lds, st, imgs + done * (int64_t)a.H * a.W,
                       a, (void*)((char*)out + done * img_out_bytes));
    OFR_LAUNCH_CHECK("lpq_kernel");
  }
  return OFR_OK;
}

// codes (counts == false: out = uint8 [n][H][W]) or fused counts (out = [n][gr*gc][256]); imgs are
// pixels of pixel_bytes: 1 (uint8), 4 (float32) or 8 (float64)
static int run(const char* who, void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int radius,
               const double* V_host, bool counts, int gr, int gc, void* out, int count_bytes) {
  const std::string w(who);
  if (n < 0 || H < 1 || W < 1) return fail(OFR_E_INVALID, w + ": bad sizes");
  if (radius < 1) return fail(OFR_E_INVALID, w + ": radius must be >= 1");
  if (radius > MAXR) return fail(OFR_E_UNSUPPORTED, w + ": radius must be <= 8");
  if (!V_host) return fail(OFR_E_INVALID, w + ": null basis");
  if (pixel_bytes != 1 && pixel_bytes != 4 && pixel_bytes != 8)
    return fail(OFR_E_INVALID, w + ": pixel_bytes must be 4 (float32) or 8 (float64)");
  if ((uintptr_t)imgs % (uintptr_t)pixel_bytes) return fail(OFR_E_INVALID, w + ": images must be aligned to their pixels");
  Args a = {};
  a.H = H;
  a.W = W;
  a.R = radius;
  a.gr = a.gc = a.py = a.px = 1;
  a.count_bytes = 1;
  a.mode = MODE_CODES;
  if (counts) {
    int rc = check_grid(who, H, W, gr, gc, out, count_bytes, a.py, a.px);
    if (rc) return rc;
    a.gr = gr;
    a.gc = gc;
    a.count_bytes = count_bytes;
    a.mode = MODE_HIST_LDS;
  }
  if (n == 0) return OFR_OK;
  if (!imgs || !out) return fail(OFR_E_INVALID, w + ": null pointer");
  if ((int64_t)H * W > MAX_PIXELS) return fail(OFR_E_UNSUPPORTED, w + ": images above 2^22 pixels");
  // strip rows: what fits beside the counters; too few, and the counters move to global memory
  const int64_t per_row = 3LL * (W + 2 * radius) * 8 + (int64_t)W * pixel_bytes;
  const int64_t halo = 2LL * radius * W * pixel_bytes + 16;
  int64_t ncnt = counts ? (int64_t)gr * gc * 256 * 4 : 0;
  int64_t SR = (LDS_BUDGET - ncnt - halo) / per_row;
  if (counts && SR < std::min(H, 4)) {
    a.mode = MODE_HIST_GLOBAL;
    ncnt = 0;
    SR = (LDS_BUDGET - halo) / per_row;
  }
  if (SR < 1) return fail(OFR_E_UNSUPPORTED, w + ": image too wide for the LDS strip");
  a.SR = (int)std::min<int64_t>(std::min<int64_t>(SR, MAX_STRIP), H);
  const size_t lds = (size_t)(ncnt + a.SR * per_row + halo);
  // few images: split each image's strips over workgroups (their counters meet in global memory)
  const int nstrips = (int)cdiv(H, a.SR);
  const int wgs = (int)std::max<int64_t>(1, std::min<int64_t>(nstrips, 1024 / n));  // n >= 513: one each
  a.strips_per_wg = (int)cdiv(nstrips, wgs);
  a.atomic_flush = cdiv(nstrips, a.strips_per_wg) > 1;
  a.inv_W = 1.0f / (float)W;
  a.inv_py = 1.0f / (float)a.py;
  a.inv_px = 1.0f / (float)a.px;
  const int nt = 2 * radius + 1;
  for (int k = 0; k < nt; ++k) {
    const double ang = 2.0 * M_PI * (double)(k - radius) / (double)nt;
    a.tap[k][0] = std::cos(ang);
    a.tap[k][1] = -std::sin(ang);
  }
  for (int j = 0; j < 8; ++j)
    for (int k = 0; k < 8; ++k) a.Vt[k][j] = V_host[8 * j + k];
  hipStream_t st = (hipStream_t)stream;
  const size_t img_out = counts ? (size_t)gr * gc * 256 * count_bytes : (size_t)H * W;
  if (a.mode == MODE_HIST_GLOBAL || (counts && a.atomic_flush)) {
    const int64_t nwords = (int64_t)n * (int64_t)(img_out / 4);
    hipLaunchKernelGGL(zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nwords, 256), 4096)), dim3(256), 0, st,
                       (uint32_t*)out, nwords);
    OFR_LAUNCH_CHECK("lpq zero_kernel");
  }
  if (pixel_bytes == 4) return launch(st, (const float*)imgs, n, a, out, lds, img_out);
  if (pixel_bytes == 8) return launch(st, (const double*)imgs, n, a, out, lds, img_out);
  return launch(st, (const uint8_t*)imgs, n, a, out, lds, img_out);
}

}  // namespace lpq
}  // namespace ofr

using namespace ofr;
using namespace ofr::lpq;

extern "C" int ofr_lpq_codes(void* stream, const uint8_t* imgs, int64_t n, int H, int W, int radius,
                             const double* V_host, uint8_t* codes) {
  return run("ofr_lpq_codes", stream, imgs, 1, n, H, W, radius, V_host, false, 1, 1, codes, 1);
}

extern "C" int ofr_lpq_codes_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int radius,
                               const double* V_host, uint8_t* codes) {
  OFR_CHECK_ARG(pixel_bytes != 1, "ofr_lpq_codes_f: pixel_bytes must be 4 (float32) or 8 (float64)");
  return run("ofr_lpq_codes_f", stream, imgs, pixel_bytes, n, H, W, radius, V_host, false, 1, 1, codes, 1);
}

extern "C" int ofr_lpq_hist(void* stream, const uint8_t* imgs, int64_t n, int H, int W, int radius,
                            const double* V_host, int gr, int gc, void* counts, int count_bytes) {
  return run("ofr_lpq_hist", stream, imgs, 1, n, H, W, radius, V_host, true, gr, gc, counts, count_bytes);
}

extern "C" int ofr_lpq_hist_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int radius,
                              const double* V_host, int gr, int gc, void* counts, int count_bytes) {
  OFR_CHECK_ARG(pixel_bytes != 1, "ofr_lpq_hist_f: pixel_bytes must be 4 (float32) or 8 (float64)");
  return run("ofr_lpq_hist_f", stream, imgs, pixel_bytes, n, H, W, radius, V_host, true, gr, gc, counts, count_bytes);
}

extern "C" int ofr_olbp_codes(void* stream, const uint8_t* imgs, int64_t n, int H, int W, uint8_t* codes) {
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1, "ofr_olbp_codes: bad sizes");
  if (n == 0 || H < 3 || W < 3) return OFR_OK;
  OFR_CHECK_ARG(imgs && codes, "ofr_olbp_codes: null pointer");
  OlbpArgs a = {};
  a.H = H;
  a.W = W;
  a.dy = H - 2;
  a.dx = W - 2;
  OFR_CHECK_ARG((int64_t)a.dy * a.dx <= 0x7fffffffLL / 2, "ofr_olbp_codes: image too large");
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv((int64_t)a.dy * cdiv(a.dx, 4), 256), 64);
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    hipLaunchKernelGGL(olbp_codes_kernel, dim3(gx, (unsigned)chunk), dim3(256), 0, (hipStream_t)stream,
                       imgs + done * (int64_t)H * W, a, codes + done * (int64_t)a.dy * a.dx);
    OFR_LAUNCH_CHECK("olbp_codes_kernel");
  }
  return OFR_OK;
}

extern "C" int ofr_olbp_hist(void* stream, const uint8_t* imgs, int64_t n, int H, int W, int gr, int gc, void* counts,
                             int count_bytes) {
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1, "ofr_olbp_hist: bad sizes");
  OlbpArgs a = {};
  a.H = H;
  a.W = W;
  a.dy = H - 2;
  a.dx = W - 2;
  a.gr = gr;
  a.gc = gc;
  a.count_bytes = count_bytes;
  int rc = check_grid("ofr_olbp_hist", a.dy, a.dx, gr, gc, counts, count_bytes, a.py, a.px);
  if (rc) return rc;
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs && counts, "ofr_olbp_hist: null pointer");
  OFR_CHECK_ARG((int64_t)a.dy * a.dx <= 0x7fffffffLL / 2, "ofr_olbp_hist: image too large");
  const int64_t lds_cap = 64 * 1024;  // bytes of u32 counters per workgroup
  const int64_t row_bytes = (int64_t)gc * 256 * 4;
  if (row_bytes > lds_cap) return fail(OFR_E_UNSUPPORTED, "ofr_olbp_hist: grid_cols too large for one LDS band");
  a.rows_per_wg = (int)std::max<int64_t>(1, std::min<int64_t>(gr, lds_cap / row_bytes));
  const unsigned gx = (unsigned)cdiv(gr, a.rows_per_wg);
  const size_t lds = (size_t)a.rows_per_wg * row_bytes;
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    hipLaunchKernelGGL(olbp_hist_kernel, dim3(gx, (unsigned)chunk), dim3(512), lds, (hipStream_t)stream,
                       imgs + done * (int64_t)H * W, a, (void*)((char*)counts + done * gr * gc * 256 * count_bytes));
    OFR_LAUNCH_CHECK("olbp_hist_kernel");
  }
  return OFR_OK;
}
