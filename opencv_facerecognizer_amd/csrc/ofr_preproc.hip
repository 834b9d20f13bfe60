// Illumination normalisation of 8-bit faces on gfx950: Tan-Triggs and histogram equalisation.
//
// Replaces TanTriggsPreprocessing.extract (reference preprocessing.py:98-105) and
// HistogramEqualization.extract (preprocessing.py:73-77) for batches of equally-sized faces.
//
// Tan-Triggs.  One workgroup of 1024 threads owns a strip of SR image rows of one face (the whole
// face when it fits: the resident form).  In LDS: the strip and its 2R halo rows as bytes (rows
// outside the image are fetched from their reflected source row, so the column pass needs no border
// rule), a 256-entry table of v^gamma (fp64 pow, rounded once to fp32), and two fp32 planes
// [SR][W|1].  Column pass (axis 0): a thread owns 8 vertically adjacent outputs of one column, walks
// the 8 + 2R bytes above and below once and feeds each v^gamma to both Gaussians, so a loaded value
// serves up to 16 taps; the two results go to the planes (the one rounding to fp32 scipy itself makes
// between its passes).  Row pass (axis 1): a thread owns 8 horizontally adjacent outputs of one row
// and walks 8 + 2R plane values (reflected at the border) of each plane; adjacent lanes take
// adjacent rows, and the odd row pitch keeps them on distinct LDS banks.  The taps are fp64 kernel
// arguments on a zero-padded common support, kept as a sliding window of 8 in scalar registers (one
// scalar load per step); all accumulation is v_fma_f64, which issues at the rate of unpacked fp32
// FMA on this chip and leaves the plane store as the only fp32 rounding of the filter.  The
// difference of Gaussians stays in registers (16 values per thread).  Both means are fixed-order
// reductions: a thread's values in order, a shuffle tree per wave, the 16 wave sums in order.
// Resident: the two scales are applied in registers, the result is staged through a plane and
// written once, coalesced -- 1 byte in, 4 bytes out per pixel, one launch.  Strips: the DoG goes to
// `out`, each strip's partial sum to the workspace; two small follow-up launches add a face's
// partials in strip order (no atomics: a face's result depends on nothing but the face), form the
// second mean the same way and finish in place -- 17 bytes per pixel.
//
// Histogram equalisation.  One workgroup of 256 threads per face: exact grey-level counts in LDS
// (the bytes are kept in LDS for the second read when the face fits), then everything is a
// 256-entry problem: min/max, numpy's uniform-bin index of every grey level present (scale,
// truncate, the two edge corrections, the last edge folded into the last bin; edges as
// np.linspace builds them: i * step + first without contraction, the last one exact), bin counts,
// density, cumulative sum in bin order, np.interp over the left edges as a 256-entry fp64 table,
// applied to every pixel.  1 byte in, 8 bytes out per pixel.
#include <cmath>

#include "ofr_common.h"

#pragma clang fp contract(off)

namespace ofr {
namespace preproc {

constexpr int LDS_BUDGET = 160 * 1024;

// ---- Tan-Triggs ---------------------------------------------------------------------------------
constexpr int MAXR = 16;       // radius = int(4 sigma + 0.5): sigma up to 4.125
constexpr int THREADS = 1024;
constexpr int RB = 8;          // outputs a thread carries along the filter axis
constexpr int TPT = 2;         // row-pass tasks (of RB pixels) a thread keeps in registers
constexpr int NTAP = 2 * MAXR + 2 * RB;  // padded taps plus the one the window loads past its last step
constexpr int FIXED_LDS = 32 * 8 + 256 * 4;  // reduction scratch + gamma table

struct Args {
  int H, W, Wp;     // Wp: odd plane pitch
  int SR, nstrips;  // rows per strip; 1 strip = resident
  int R;            // common support radius max(R0, R1)
  int lo0, hi0, lo1, hi1;  // steps j of the 8 + 2R walk at which filter 0 / 1 has a non-zero tap
  float inv_W, alpha, tau;
  double gamma, inv_alpha;
  double w0[NTAP], w1[NTAP];  // tap k of the common support at [k + RB - 1], zero elsewhere
};

// a / d for 0 <= a < 2^22, inv = 1.0f / d
__device__ __forceinline__ int fdiv(int a, int d, float inv) {
  int q = (int)((float)a * inv);
  const int r = a - q * d;
  if (r < 0) --q;
  else if (r >= d) ++q;
  return q;
}

// scipy's 'reflect' border: -1 -> 0, -2 -> 1, n -> n - 1; repeats with period 2n
__device__ __forceinline__ int reflect(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -1 - i : 2 * n - 1 - i;
  return i;
}

__device__ __forceinline__ float powa(float x, float alpha) { return exp2f(alpha * log2f(x)); }  // x >= 0; 0 -> 0

// sum of v over the workgroup in a fixed order, returned to every thread
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();  // the previous sum has been read
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < nw; ++w) s += red[w];
  return s;
}

// one Gaussian over RB + 2R steps: acc[o] += w[j - o] * v, the taps as a sliding scalar window
#define OFR_TT_WINDOW_INIT(ww, w)             \
  _Pragma("unroll") for (int o = 0; o < RB; ++o) ww[o] = w[RB - 1 - o]
#define OFR_TT_WINDOW_STEP(ww, w, j)                          \
  _Pragma("unroll") for (int o = RB - 1; o > 0; --o) ww[o] = ww[o - 1]; \
  ww[0] = w[(j) + RB]

__global__ void __launch_bounds__(THREADS) tantriggs_kernel(const uint8_t* __restrict__ imgs, Args a,
                                                            float* __restrict__ out, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int H = a.H, W = a.W, Wp = a.Wp, R = a.R;
  double* red = reinterpret_cast<double*>(smem);
  float* lut = reinterpret_cast<float*>(smem + 32 * 8);
  float* P1 = lut + 256;
  float* P0 = P1 + a.SR * Wp;
  uint8_t* tile = reinterpret_cast<uint8_t*>(P0 + a.SR * Wp);  // [rows + 2R][W]
  const int64_t img = blockIdx.y;
  const int64_t npix = (int64_t)H * W;
  const uint8_t* im = imgs + img * npix;
  float* o_img = out + img * npix;
  const int y0 = blockIdx.x * a.SR, rows = min(a.SR, H - y0), trow = rows + 2 * R;
  const int tid = threadIdx.x;

  if (tid < 256) lut[tid] = (float)pow((double)tid, a.gamma);
  for (int i = tid; i < trow * W; i += THREADS) {
    const int t = fdiv(i, W, a.inv_W), x = i - t * W;
    tile[i] = im[(int64_t)reflect(y0 - R + t, H) * W + x];
  }
  __syncthreads();

  // column pass: plane(y, x) = sum_k w[k] X(y + k - R, x); tile row of image row y0 + y + k - R is y + k
  const int nrb = (rows + RB - 1) / RB;
  for (int t = tid; t < nrb * W; t += THREADS) {
    const int rb = fdiv(t, W, a.inv_W), x = t - rb * W;
    const int yb = rb * RB;
    const int jn = min(RB + 2 * R, trow - yb);
    const uint8_t* col = tile + yb * W + x;
    double a1[RB], a0[RB], u1[RB], u0[RB];
#pragma unroll
    for (int o = 0; o < RB; ++o) a1[o] = a0[o] = 0.0;
    OFR_TT_WINDOW_INIT(u1, a.w1);
    OFR_TT_WINDOW_INIT(u0, a.w0);
    for (int j = 0; j < jn; ++j) {
      const double v = (double)lut[col[j * W]];
      if (j >= a.lo1 && j < a.hi1) {
#pragma unroll
        for (int o = 0; o < RB; ++o) a1[o] = fma(u1[o], v, a1[o]);
      }
      if (j >= a.lo0 && j < a.hi0) {
#pragma unroll
        for (int o = 0; o < RB; ++o) a0[o] = fma(u0[o], v, a0[o]);
      }
      OFR_TT_WINDOW_STEP(u1, a.w1, j);
      OFR_TT_WINDOW_STEP(u0, a.w0, j);
    }
#pragma unroll
    for (int o = 0; o < RB; ++o) {
      if (yb + o < rows) {
        P1[(yb + o) * Wp + x] = (float)a1[o];
        P0[(yb + o) * Wp + x] = (float)a0[o];
      }
    }
  }
  __syncthreads();

  // row pass: D(y, x) = sum_k w1[k] P1(y, x + k - R) - sum_k w0[k] P0(y, x + k - R), columns reflected
  const int ncb = (W + RB - 1) / RB;
  const float inv_rows = 1.0f / (float)rows;
  double D[TPT][RB];
  int px[TPT], xbs[TPT];  // plane index and column of a task's first pixel; column W: no task
#pragma unroll
  for (int s = 0; s < TPT; ++s) {
    const int t = tid + s * THREADS;
    px[s] = 0;
    xbs[s] = W;
#pragma unroll
    for (int o = 0; o < RB; ++o) D[s][o] = 0.0;
    if (t < ncb * rows) {
      const int cb = fdiv(t, rows, inv_rows), y = t - cb * rows;
      const int xb = cb * RB;
      px[s] = y * Wp + xb;
      xbs[s] = xb;
      double a1[RB], a0[RB], u1[RB], u0[RB];
#pragma unroll
      for (int o = 0; o < RB; ++o) a1[o] = a0[o] = 0.0;
      OFR_TT_WINDOW_INIT(u1, a.w1);
      OFR_TT_WINDOW_INIT(u0, a.w0);
      for (int j = 0; j < RB + 2 * R; ++j) {
        const int c = y * Wp + reflect(xb - R + j, W);
        if (j >= a.lo1 && j < a.hi1) {
          const double v = (double)P1[c];
#pragma unroll
          for (int o = 0; o < RB; ++o) a1[o] = fma(u1[o], v, a1[o]);
        }
        if (j >= a.lo0 && j < a.hi0) {
          const double v = (double)P0[c];
#pragma unroll
          for (int o = 0; o < RB; ++o) a0[o] = fma(u0[o], v, a0[o]);
        }
        OFR_TT_WINDOW_STEP(u1, a.w1, j);
        OFR_TT_WINDOW_STEP(u0, a.w0, j);
      }
#pragma unroll
      for (int o = 0; o < RB; ++o) D[s][o] = a1[o] - a0[o];
    }
  }

  // first mean: sum |D|^alpha over the thread's pixels (columns past W carry no pixel)
  double part = 0.0;
#pragma unroll
  for (int s = 0; s < TPT; ++s) {
    const int xb = xbs[s];
#pragma unroll
    for (int o = 0; o < RB; ++o)
      if (xb + o < W) part += (double)powa((float)fabs(D[s][o]), a.alpha);
  }
  double total = block_sum(part, red);  // (its barriers also end the row pass's reads of the planes)
  if (a.nstrips == 1) {
    const double r1 = 1.0 / pow(total / (double)npix, a.inv_alpha);  // one divide per face, not per pixel
    part = 0.0;
#pragma unroll
    for (int s = 0; s < TPT; ++s) {
      const int xb = xbs[s];
#pragma unroll
      for (int o = 0; o < RB; ++o) {
        D[s][o] = D[s][o] * r1;
        if (xb + o < W) part += (double)powa(fminf((float)fabs(D[s][o]), a.tau), a.alpha);
      }
    }
    total = block_sum(part, red);
    const double r2 = 1.0 / pow(total / (double)npix, a.inv_alpha);
    const float rtau = 1.0f / a.tau;
#pragma unroll
    for (int s = 0; s < TPT; ++s)
#pragma unroll
      for (int o = 0; o < RB; ++o) D[s][o] = (double)(a.tau * tanhf((float)(D[s][o] * r2) * rtau));
  } else if (tid == 0) {
    ws[img * a.nstrips + blockIdx.x] = total;
  }
  // stage through plane 1, then one coalesced store of the strip
#pragma unroll
  for (int s = 0; s < TPT; ++s) {
    const int xb = xbs[s];
#pragma unroll
    for (int o = 0; o < RB; ++o)
      if (xb + o < W) P1[px[s] + o] = (float)D[s][o];
  }
  __syncthreads();
  for (int i = tid; i < rows * W; i += THREADS) {
    const int y = fdiv(i, W, a.inv_W), x = i - y * W;
    o_img[(int64_t)y0 * W + i] = P1[y * Wp + x];
  }
}

// strips only.  phase 0: the face's first scale from its strip partials, this strip's partial of the
// second mean -> ws2; phase 1: both scales, the result in place.
__global__ void __launch_bounds__(THREADS) tantriggs_finish_kernel(Args a, int phase, float* __restrict__ out,
                                                                   const double* __restrict__ ws1,
                                                                   double* __restrict__ ws2) {
  __shared__ double red[32];
  const int64_t img = blockIdx.y;
  const int64_t npix = (int64_t)a.H * a.W;
  const int y0 = blockIdx.x * a.SR, rows = min(a.SR, a.H - y0);
  float* d = out + img * npix + (int64_t)y0 * a.W;
  double t1 = 0.0, t2 = 0.0;
  for (int s = 0; s < a.nstrips; ++s) t1 += ws1[img * a.nstrips + s];
  const double r1 = 1.0 / pow(t1 / (double)npix, a.inv_alpha);
  if (phase == 0) {
    double part = 0.0;
    for (int i = threadIdx.x; i < rows * a.W; i += THREADS)
      part += (double)powa(fminf((float)fabs((double)d[i] * r1), a.tau), a.alpha);
    const double total = block_sum(part, red);
    if (threadIdx.x == 0) ws2[img * a.nstrips + blockIdx.x] = total;
    return;
  }
  for (int s = 0; s < a.nstrips; ++s) t2 += ws2[img * a.nstrips + s];
  const double r2 = 1.0 / pow(t2 / (double)npix, a.inv_alpha);
  const float rtau = 1.0f / a.tau;
  for (int i = threadIdx.x; i < rows * a.W; i += THREADS)
    d[i] = a.tau * tanhf((float)(((double)d[i] * r1) * r2) * rtau);
}

static size_t tt_lds(int rows, int W, int R) {
  return (size_t)FIXED_LDS + 2 * (size_t)rows * (W | 1) * 4 + (size_t)(rows + 2 * R) * W + 16;
}

// rows per strip: the whole face when its row-pass tasks fit the threads' registers and its planes the
// LDS; else the largest multiple of RB that does (0: the image is too wide)
static int tt_strip_rows(int H, int W, int R) {
  const int64_t ncb = cdiv(W, RB);
  auto fits = [&](int64_t rows) { return rows * ncb <= (int64_t)TPT * THREADS && tt_lds((int)rows, W, R) <= (size_t)LDS_BUDGET; };
  if (fits(H)) return H;
  int64_t sr = std::min<int64_t>(H, (int64_t)TPT * THREADS / ncb);
  while (sr > 0 && !fits(sr)) --sr;
  if (sr > RB) sr -= sr % RB;
  return (int)sr;
}

static int radius_of(double sigma) { return (int)(4.0 * sigma + 0.5); }

// scipy's _gaussian_kernel1d (order 0) of radius r on the common support of radius R, zero-padded by RB - 1
static void fill_taps(double* w, double sigma, int r, int R) {
  for (int i = 0; i < NTAP; ++i) w[i] = 0.0;
  double sum = 0.0;
  for (int x = -r; x <= r; ++x) sum += std::exp(-0.5 / (sigma * sigma) * (double)(x * x));
  for (int x = -r; x <= r; ++x) w[x + R + RB - 1] = std::exp(-0.5 / (sigma * sigma) * (double)(x * x)) / sum;
}

// ---- histogram equalisation -----------------------------------------------------------------------
constexpr int HE_THREADS = 256;
constexpr int HE_MAXBINS = 4096;

__global__ void __launch_bounds__(HE_THREADS) histeq_kernel(const uint8_t* __restrict__ imgs, int64_t npix, int nb,
                                                            int keep, double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* cdf = reinterpret_cast<double*>(smem);      // [nb]
  double* lut = cdf + nb;                             // [256]
  uint32_t* bins = reinterpret_cast<uint32_t*>(lut + 256);  // [nb]
  uint32_t* hist = bins + nb;                         // [256]
  int* mm = reinterpret_cast<int*>(hist + 256);       // min, max grey level
  uint8_t* pix = reinterpret_cast<uint8_t*>(mm + 4);  // [npix] when keep
  const int tid = threadIdx.x;
  const uint8_t* im = imgs + (int64_t)blockIdx.x * npix;
  double* o = out + (int64_t)blockIdx.x * npix;

  hist[tid] = 0;
  for (int b = tid; b < nb; b += HE_THREADS) bins[b] = 0;
  if (tid == 0) {
    mm[0] = 255;
    mm[1] = 0;
  }
  __syncthreads();
  if ((npix & 3) == 0 && ((uintptr_t)im & 3) == 0) {
    for (int64_t i = tid; i < npix / 4; i += HE_THREADS) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(im)[i];
      if (keep) reinterpret_cast<uint32_t*>(pix)[i] = w;
      atomicAdd(&hist[w & 0xffu], 1u);
      atomicAdd(&hist[(w >> 8) & 0xffu], 1u);
      atomicAdd(&hist[(w >> 16) & 0xffu], 1u);
      atomicAdd(&hist[w >> 24], 1u);
    }
  } else {
    for (int64_t i = tid; i < npix; i += HE_THREADS) {
      const uint8_t b = im[i];
      if (keep) pix[i] = b;
      atomicAdd(&hist[b], 1u);
    }
  }
  __syncthreads();
  const uint32_t cnt = hist[tid];
  if (cnt) {
    atomicMin(&mm[0], tid);
    atomicMax(&mm[1], tid);
  }
  __syncthreads();
  // np.histogram's outer edges and np.linspace's inner ones
  const int lo = mm[0], hi = mm[1];
  double first = (double)lo, last = (double)hi, denom = (double)(hi - lo);
  if (lo == hi) {
    first = first - 0.5;
    last = last + 0.5;
    denom = last - first;
  }
  const double step = (last - first) / (double)nb;
#define OFR_HE_EDGE(i) ((i) == nb ? last : (double)(i) * step + first)
  if (cnt) {  // the uniform-bin index of grey level tid
    const double v = (double)tid;
    int idx = (int)(((v - first) / denom) * (double)nb);
    if (idx == nb) --idx;
    if (v < OFR_HE_EDGE(idx)) --idx;
    if (v >= OFR_HE_EDGE(idx + 1) && idx != nb - 1) ++idx;
    atomicAdd(&bins[idx], cnt);
  }
  __syncthreads();
  for (int b = tid; b < nb; b += HE_THREADS)  // density: n / db / n.sum()
    cdf[b] = ((double)bins[b] / (OFR_HE_EDGE(b + 1) - OFR_HE_EDGE(b))) / (double)npix;
  __syncthreads();
  if (tid == 0) {  // cumsum in bin order
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) cdf[b] = acc = acc + cdf[b];
  }
  __syncthreads();
  const double top = cdf[nb - 1];
  __syncthreads();
  for (int b = tid; b < nb; b += HE_THREADS) cdf[b] = 255.0 * cdf[b] / top;
  __syncthreads();
  {  // np.interp(tid, edges[:-1], cdf)
    const double v = (double)tid;
    double r;
    if (v <= OFR_HE_EDGE(0)) {
      r = cdf[0];
    } else if (v >= OFR_HE_EDGE(nb - 1)) {
      r = cdf[nb - 1];
    } else {
      int j = 0, j1 = nb - 1;  // edge(j) <= v < edge(j1)
      while (j1 - j > 1) {
        const int m = (j + j1) >> 1;
        if (v >= OFR_HE_EDGE(m)) j = m;
        else j1 = m;
      }
      const double e0 = OFR_HE_EDGE(j), e1 = OFR_HE_EDGE(j + 1);
      r = ((cdf[j + 1] - cdf[j]) / (e1 - e0)) * (v - e0) + cdf[j];
    }
    lut[tid] = r;
  }
#undef OFR_HE_EDGE
  __syncthreads();
  if (keep) {
    for (int64_t i = tid; i < npix; i += HE_THREADS) o[i] = lut[pix[i]];
  } else {
    for (int64_t i = tid; i < npix; i += HE_THREADS) o[i] = lut[im[i]];
  }
}

}  // namespace preproc
}  // namespace ofr

using namespace ofr;
using namespace ofr::preproc;

static int tt_plan(const char* who, int64_t n, int H, int W, double alpha, double tau, double gamma, double sigma0,
                   double sigma1, Args& a) {
  const std::string w(who);
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1, w + ": bad sizes");
  OFR_CHECK_ARG(sigma0 > 0 && sigma1 > 0 && alpha > 0 && tau > 0, w + ": sigma0, sigma1, alpha and tau must be > 0");
  OFR_CHECK_ARG(std::isfinite(alpha) && std::isfinite(tau) && std::isfinite(gamma), w + ": non-finite parameter");
  OFR_CHECK_ARG(sigma0 <= 1e6 && sigma1 <= 1e6, w + ": sigma too large");
  const int R0 = radius_of(sigma0), R1 = radius_of(sigma1);
  OFR_CHECK_ARG(R0 <= MAXR && R1 <= MAXR, w + ": filter radius int(4 sigma + 0.5) must be <= 16");
  a = Args{};
  a.H = H;
  a.W = W;
  a.Wp = W | 1;
  a.R = std::max(R0, R1);
  a.SR = tt_strip_rows(H, W, a.R);
  if (a.SR < 1) return fail(OFR_E_UNSUPPORTED, w + ": image too wide for the LDS strip");
  a.nstrips = (int)cdiv(H, a.SR);
  a.lo0 = a.R - R0;
  a.hi0 = a.R + R0 + RB;
  a.lo1 = a.R - R1;
  a.hi1 = a.R + R1 + RB;
  a.inv_W = 1.0f / (float)W;
  a.alpha = (float)alpha;
  a.tau = (float)tau;
  a.gamma = gamma;
  a.inv_alpha = 1.0 / alpha;
  fill_taps(a.w0, sigma0, R0, a.R);
  fill_taps(a.w1, sigma1, R1, a.R);
  return OFR_OK;
}

extern "C" size_t ofr_tantriggs_workspace_bytes(int64_t n, int H, int W, double sigma0, double sigma1) {
  Args a;
  if (tt_plan("ofr_tantriggs_workspace_bytes", n, H, W, 1.0, 1.0, 1.0, sigma0, sigma1, a) != OFR_OK) return 0;
  return a.nstrips == 1 ? 0 : (size_t)2 * n * a.nstrips * sizeof(double);
}

extern "C" int ofr_tantriggs_f32(void* stream, const uint8_t* imgs, int64_t n, int H, int W, double alpha, double tau,
                                 double gamma, double sigma0, double sigma1, float* out, void* workspace,
                                 size_t workspace_bytes) {
  Args a;
  int rc = tt_plan("ofr_tantriggs_f32", n, H, W, alpha, tau, gamma, sigma0, sigma1, a);
  if (rc) return rc;
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs && out, "ofr_tantriggs_f32: null pointer");
  const bool strips = a.nstrips > 1;
  const size_t need = strips ? (size_t)2 * n * a.nstrips * sizeof(double) : 0;
  OFR_CHECK_ARG(!strips || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
                "ofr_tantriggs_f32: workspace too small (ofr_tantriggs_workspace_bytes)");
  static bool attr = false;
  if (!attr) {
    hipError_t e =
        hipFuncSetAttribute((const void*)tantriggs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BUDGET);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(tantriggs_kernel)");
    attr = true;
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = tt_lds(a.SR, W, a.R);
  const int64_t npix = (int64_t)H * W;
  double* ws1 = (double*)workspace;
  double* ws2 = ws1 ? ws1 + n * a.nstrips : nullptr;
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    const dim3 grid((unsigned)a.nstrips, (unsigned)chunk);
    double* w1 = strips ? ws1 + done * a.nstrips : nullptr;
    double* w2 = strips ? ws2 + done * a.nstrips : nullptr;
    hipLaunchKernelGGL(tantriggs_kernel, grid, dim3(THREADS), lds, st, imgs + done * npix, a, out + done * npix, w1);
    OFR_LAUNCH_CHECK("tantriggs_kernel");
    if (!strips) continue;
    for (int phase = 0; phase < 2; ++phase) {
      hipLaunchKernelGGL(tantriggs_finish_kernel, grid, dim3(THREADS), 0, st, a, phase, out + done * npix, w1, w2);
      OFR_LAUNCH_CHECK("tantriggs_finish_kernel");
    }
  }
  return OFR_OK;
}

extern "C" int ofr_histeq_f64(void* stream, const uint8_t* imgs, int64_t n, int H, int W, int num_bins, double* out) {
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1, "ofr_histeq_f64: bad sizes");
  OFR_CHECK_ARG(num_bins >= 1 && num_bins <= HE_MAXBINS, "ofr_histeq_f64: num_bins must be 1..4096");
  OFR_CHECK_ARG(n <= 0x7fffffffLL, "ofr_histeq_f64: too many images");
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs && out, "ofr_histeq_f64: null pointer");
  const int64_t npix = (int64_t)H * W;
  OFR_CHECK_ARG(npix <= 0x7fffffffLL, "ofr_histeq_f64: image too large");
  const size_t fixed = (size_t)num_bins * 12 + 256 * 12 + 16;
  const int keep = fixed + (size_t)npix + 16 <= (size_t)64 * 1024;  // 64 KiB: the default limit, several faces per CU
  const size_t lds = fixed + (keep ? (size_t)round_up(npix, 4) : 0);
  hipLaunchKernelGGL(histeq_kernel, dim3((unsigned)n), dim3(HE_THREADS), lds, (hipStream_t)stream, imgs, npix, num_bins,
                     keep, out);
  OFR_LAUNCH_CHECK("histeq_kernel");
  return OFR_OK;
}
