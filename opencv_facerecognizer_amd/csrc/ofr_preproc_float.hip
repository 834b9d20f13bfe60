// Illumination normalisation of float32 / float64 faces on gfx950: Tan-Triggs and histogram
// equalisation.  The float twins of ofr_preproc.hip: what one preprocessing step returns (Tan-Triggs:
// float32 in (-tau, tau); equalisation: float64 in 0..255) or what the caller holds as float faces goes
// through the other step without a host trip.
//
// Semantics.  Tan-Triggs (reference preprocessing.py:98-105): every pixel is rounded once to float32
// (np.array(X, dtype=np.float32)), v^gamma is float32, then the byte kernel's arithmetic to the letter:
// two Gaussians with fp64 taps and fma accumulation, one fp32 rounding between the two passes, the two
// means as fixed-order reductions, the two scalings, tanh.  Equalisation (preprocessing.py:73-77):
// np.histogram / np.interp as numpy 2.x evaluates them on an array of THAT dtype -- for a float32 image
// the outer edges, np.linspace's inner edges, the index arithmetic and the two edge corrections are
// all float32 (bin_edges.dtype is float32), for a float64 image fp64; from the counts on everything is
// fp64 for both (np.diff of the edges is taken in the edges' type and then widened).
//
// Design.  The byte kernels rest on the pixel being one byte (a 256-entry power table, a byte strip,
// grey-level counts, a 256-entry interpolation table); none of that survives a float pixel.
//
// Tan-Triggs.  One workgroup of 1024 threads owns a strip of SR image rows of one face (the whole face
// when it fits: the resident form).  LDS: the strip and its 2R halo rows as FP32 v^gamma, two fp32
// planes [SR][W|1], 32 doubles of reduction scratch.
// * Staging converts and raises to the power.  The strip's rows that lie inside the image are
//   contiguous in memory; they are loaded 16 bytes at a time (4 float32 / 2 float64) from the first
//   16-byte boundary of the strip on, the elements in front of it and behind the last whole vector one
//   by one (alignment is a property of the strip's first byte, not of the row pitch).  The thread that
//   loaded a pixel rounds it to float32 and computes v^gamma once: exp2(gamma * log2(v)) in fp64,
//   rounded once to fp32 (relative error of the fp64 value below 1e-13 for every float32 v > 0, so the
//   result is the correctly rounded float32 power but for about one value in 10^6, where it is the
//   neighbour; 0 -> 0, a negative pixel -> NaN as in the reference).  Halo rows outside the image are
//   then copied LDS -> LDS from their reflected source row, which always lies inside the staged rows:
//   the power is never computed twice within a strip, and the column pass needs no border rule and reads
//   LDS exactly as often as the byte kernel does -- a float where that reads a byte and a table entry.
// * Column pass, row pass, the sliding scalar tap window, the register-resident difference of
//   Gaussians, the reductions and the coalesced store through plane 1: as in ofr_preproc.hip.
// * Strips: as there -- the DoG to `out`, per-strip partial sums to the workspace, two follow-up
//   launches that add them in strip order.  The strip count differs from the byte kernel's (4-byte
//   strip plane), so the workspace has its own size function, ofr_tantriggs_workspace_bytes_f.
// * LDS budget: 12 bytes per strip pixel + 4 W bytes per halo row (the byte kernel: 9 and W).  A face
//   is resident when it fits the 160 KiB of a workgroup: 113 x 113 at the default sigmas (R = 8), against
//   the byte kernel's 128 x 128 (which its registers limit, not its LDS); 79 x 79 and smaller need no
//   more than 80 KiB.  A larger face runs in strips of the largest multiple of 8 rows that fits 160 KiB
//   (the kernel's register count allows one workgroup per CU, so a strip sized for 80 KiB would only
//   add halo rows).
//
// Equalisation.  One workgroup of 512 threads per face, pixel type T = float or double.
// * Read 1 (16-byte loads, same rule): the face goes to LDS as T when it fits (<= 160 KiB with the
//   tables), each thread keeps min / max of what it loaded; a shuffle tree per wave and the 8 wave
//   results in order give the face's range.
// * Every pixel gets its own bin index, in T and in numpy's order: subtract, divide by the range,
//   multiply by num_bins, truncate, fold == num_bins, decrement / increment against the edges
//   (i * step + first without contraction, the last edge exact).  Counts are LDS atomics on integers.
// * Density, cumulative sum in bin order by one thread, 255 cdf / cdf[-1]: fp64 as in the byte kernel.
// * Read 2 (from LDS, else from memory again): np.interp per pixel over the num_bins left edges.
//   They are uniform, so the interval comes from one fp64 multiply, (v - first) * (num_bins / range),
//   and is then walked down / up against the edges themselves until edge[j] <= v < edge[j + 1]: the
//   walk makes it searchsorted's answer whatever the multiply's rounding was, and takes 0 or 1 steps.
// A face that does not fit LDS is read three times (range, counts, output).
#include <cmath>

#include "ofr_common.h"

#pragma clang fp contract(off)

namespace ofr {
namespace preprocf {

constexpr int LDS_MAX = 160 * 1024;

// ---- Tan-Triggs ---------------------------------------------------------------------------------
constexpr int MAXR = 16;       // radius = int(4 sigma + 0.5): sigma up to 4.125
constexpr int THREADS = 1024;
constexpr int RB = 8;          // outputs a thread carries along the filter axis
constexpr int TPT = 2;         // row-pass tasks (of RB pixels) a thread keeps in registers
constexpr int NTAP = 2 * MAXR + 2 * RB;  // padded taps plus the one the window loads past its last step
constexpr int FIXED_LDS = 32 * 8;        // reduction scratch

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

// np.power(float32 v, gamma) for v >= 0: fp64, rounded once (v < 0: NaN; gamma == 0: 1 like pow)
__device__ __forceinline__ float powg(float v, double gamma) {
  return gamma == 0.0 ? 1.0f : (float)exp2(gamma * log2((double)v));
}

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

// `count` contiguous pixels -> fp32 v^gamma in LDS; 16-byte loads from the first 16-byte boundary on
template <typename T>
__device__ __forceinline__ void stage_power(const T* __restrict__ src, float* __restrict__ dst, int count,
                                            double gamma) {
  constexpr int V = 16 / (int)sizeof(T);
  const int head = min(count, (int)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) / sizeof(T)));
  const int nvec = (count - head) / V;
  for (int i = threadIdx.x; i < head; i += THREADS) dst[i] = powg((float)src[i], gamma);
  const T* body = src + head;
  float* o = dst + head;
  for (int i = threadIdx.x; i < nvec; i += THREADS) {
    if constexpr (sizeof(T) == 4) {
      const float4 v = reinterpret_cast<const float4*>(body)[i];
      o[4 * i + 0] = powg(v.x, gamma);
      o[4 * i + 1] = powg(v.y, gamma);
      o[4 * i + 2] = powg(v.z, gamma);
      o[4 * i + 3] = powg(v.w, gamma);
    } else {
      const double2 v = reinterpret_cast<const double2*>(body)[i];
      o[2 * i + 0] = powg((float)v.x, gamma);
      o[2 * i + 1] = powg((float)v.y, gamma);
    }
  }
  for (int i = head + nvec * V + threadIdx.x; i < count; i += THREADS) dst[i] = powg((float)src[i], gamma);
}

// one Gaussian over RB + 2R steps: acc[o] += w[j - o] * v, the taps as a sliding scalar window
#define OFR_TTF_WINDOW_INIT(ww, w)            \
  _Pragma("unroll") for (int o = 0; o < RB; ++o) ww[o] = w[RB - 1 - o]
#define OFR_TTF_WINDOW_STEP(ww, w, j)                         \
  _Pragma("unroll") for (int o = RB - 1; o > 0; --o) ww[o] = ww[o - 1]; \
  ww[0] = w[(j) + RB]

template <typename T>
__global__ void __launch_bounds__(THREADS) tantriggs_kernel(const T* __restrict__ imgs, Args a,
                                                            float* __restrict__ out, double* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int H = a.H, W = a.W, Wp = a.Wp, R = a.R;
  double* red = reinterpret_cast<double*>(smem);
  float* P1 = reinterpret_cast<float*>(smem + FIXED_LDS);
  float* P0 = P1 + a.SR * Wp;
  float* tile = P0 + a.SR * Wp;  // [rows + 2R][W] of v^gamma
  const int64_t img = blockIdx.y;
  const int64_t npix = (int64_t)H * W;
  const T* im = imgs + img * npix;
  float* o_img = out + img * npix;
  const int y0 = blockIdx.x * a.SR, rows = min(a.SR, H - y0), trow = rows + 2 * R;
  const int tid = threadIdx.x;

  // tile row t holds image row y0 - R + t; rows [ya, yb) of the image are in range and contiguous
  const int ya = max(0, y0 - R), yb = min(H, y0 + rows + R);
  const int t0 = ya - (y0 - R), t1 = t0 + (yb - ya);
  stage_power(im + (int64_t)ya * W, tile + t0 * W, (yb - ya) * W, a.gamma);
  __syncthreads();
  // halo rows outside the image: their reflected source row is one of the staged rows
  for (int i = tid; i < t0 * W; i += THREADS) {
    const int t = fdiv(i, W, a.inv_W), x = i - t * W;
    tile[i] = tile[(reflect(y0 - R + t, H) - ya + t0) * W + x];
  }
  for (int i = t1 * W + tid; i < trow * W; i += THREADS) {
    const int t = fdiv(i, W, a.inv_W), x = i - t * W;
    tile[i] = tile[(reflect(y0 - R + t, H) - ya + t0) * W + x];
  }
  __syncthreads();

  // column pass: plane(y, x) = sum_k w[k] X(y + k - R, x); tile row of image row y0 + y + k - R is y + k
  const int nrb = (rows + RB - 1) / RB;
  for (int t = tid; t < nrb * W; t += THREADS) {
    const int rb = fdiv(t, W, a.inv_W), x = t - rb * W;
    const int yb8 = rb * RB;
    const int jn = min(RB + 2 * R, trow - yb8);
    const float* col = tile + yb8 * W + x;
    double a1[RB], a0[RB], u1[RB], u0[RB];
#pragma unroll
    for (int o = 0; o < RB; ++o) a1[o] = a0[o] = 0.0;
    OFR_TTF_WINDOW_INIT(u1, a.w1);
    OFR_TTF_WINDOW_INIT(u0, a.w0);
    for (int j = 0; j < jn; ++j) {
      const double v = (double)col[j * W];
      if (j >= a.lo1 && j < a.hi1) {
#pragma unroll
        for (int o = 0; o < RB; ++o) a1[o] = fma(u1[o], v, a1[o]);
      }
      if (j >= a.lo0 && j < a.hi0) {
#pragma unroll
        for (int o = 0; o < RB; ++o) a0[o] = fma(u0[o], v, a0[o]);
      }
      OFR_TTF_WINDOW_STEP(u1, a.w1, j);
      OFR_TTF_WINDOW_STEP(u0, a.w0, j);
    }
#pragma unroll
    for (int o = 0; o < RB; ++o) {
      if (yb8 + o < rows) {
        P1[(yb8 + o) * Wp + x] = (float)a1[o];
        P0[(yb8 + o) * Wp + x] = (float)a0[o];
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
      OFR_TTF_WINDOW_INIT(u1, a.w1);
      OFR_TTF_WINDOW_INIT(u0, a.w0);
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
        OFR_TTF_WINDOW_STEP(u1, a.w1, j);
        OFR_TTF_WINDOW_STEP(u0, a.w0, j);
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
  return (size_t)FIXED_LDS + 2 * (size_t)rows * (W | 1) * 4 + (size_t)(rows + 2 * R) * W * 4;
}

// rows per strip: the whole face when its row-pass tasks fit the threads' registers and its planes the
// LDS; else the largest multiple of RB that does (0: the image is too wide)
static int tt_strip_rows(int H, int W, int R) {
  const int64_t ncb = cdiv(W, RB);
  auto fits = [&](int64_t rows) { return rows * ncb <= (int64_t)TPT * THREADS && tt_lds((int)rows, W, R) <= (size_t)LDS_MAX; };
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
constexpr int HE_THREADS = 512;
constexpr int HE_WAVES = HE_THREADS / 64;
constexpr int HE_MAXBINS = 4096;
constexpr int HE_FIXED = 2 * HE_WAVES * 8;  // the waves' min / max, in 8-byte slots

// np.histogram's uniform bins in the image's own type T
template <typename T>
struct Bins {
  T first, last, denom, step;
  int nb;
  __device__ __forceinline__ T edge(int i) const { return i == nb ? last : (T)i * step + first; }  // np.linspace
  // the uniform-bin branch of np.histogram, clamped so that no value, finite or not, leaves [0, nb)
  __device__ __forceinline__ int index(T v) const {
    T f = ((v - first) / denom) * (T)nb;
    f = f >= (T)0 ? f : (T)0;
    f = f <= (T)nb ? f : (T)nb;
    int idx = (int)f;
    if (idx == nb) --idx;
    if (v < edge(idx)) --idx;
    idx = max(idx, 0);
    if (v >= edge(idx + 1) && idx != nb - 1) ++idx;
    return idx;
  }
};

// process `count` contiguous pixels, 16-byte loads from the first 16-byte boundary on: f(index, value)
template <typename T, typename F>
__device__ __forceinline__ void for_pixels(const T* __restrict__ src, int count, F f) {
  constexpr int V = 16 / (int)sizeof(T);
  const int head = min(count, (int)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) / sizeof(T)));
  const int nvec = (count - head) / V;
  for (int i = threadIdx.x; i < head; i += HE_THREADS) f(i, src[i]);
  const T* body = src + head;
  for (int i = threadIdx.x; i < nvec; i += HE_THREADS) {
    if constexpr (sizeof(T) == 4) {
      const float4 v = reinterpret_cast<const float4*>(body)[i];
      f(head + 4 * i + 0, v.x);
      f(head + 4 * i + 1, v.y);
      f(head + 4 * i + 2, v.z);
      f(head + 4 * i + 3, v.w);
    } else {
      const double2 v = reinterpret_cast<const double2*>(body)[i];
      f(head + 2 * i + 0, v.x);
      f(head + 2 * i + 1, v.y);
    }
  }
  for (int i = head + nvec * V + threadIdx.x; i < count; i += HE_THREADS) f(i, src[i]);
}

template <typename T>
__global__ void __launch_bounds__(HE_THREADS) histeq_kernel(const T* __restrict__ imgs, int npix, int nb, int keep,
                                                            double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* cdf = reinterpret_cast<double*>(smem);              // [nb]
  T* wmin = reinterpret_cast<T*>(cdf + nb);                   // [HE_WAVES]
  T* wmax = reinterpret_cast<T*>(cdf + nb + HE_WAVES);        // [HE_WAVES]
  uint32_t* bins = reinterpret_cast<uint32_t*>(cdf + nb + 2 * HE_WAVES);  // [nb], padded to 8 bytes
  T* pix = reinterpret_cast<T*>(bins + ((nb + 1) & ~1));      // [npix] when keep
  const int tid = threadIdx.x;
  const T* im = imgs + (int64_t)blockIdx.x * npix;
  double* o = out + (int64_t)blockIdx.x * npix;

  // read 1: the face's range, the face to LDS
  T lo = im[0], hi = lo;
  for (int b = tid; b < nb; b += HE_THREADS) bins[b] = 0;
  for_pixels(im, npix, [&](int i, T v) {
    if (keep) pix[i] = v;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  });
  for (int off = 32; off > 0; off >>= 1) {
    const T l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((tid & 63) == 0) {
    wmin[tid >> 6] = lo;
    wmax[tid >> 6] = hi;
  }
  __syncthreads();
  lo = wmin[0];
  hi = wmax[0];
  for (int w = 1; w < HE_WAVES; ++w) {
    lo = wmin[w] < lo ? wmin[w] : lo;
    hi = wmax[w] > hi ? wmax[w] : hi;
  }
  // np.histogram's outer edges (_get_outer_edges) and np.linspace's step, all in T
  Bins<T> B;
  B.nb = nb;
  B.first = lo;
  B.last = hi;
  if (lo == hi) {
    B.first = lo - (T)0.5;
    B.last = hi + (T)0.5;
  }
  B.denom = B.last - B.first;
  B.step = B.denom / (T)nb;

  if (keep) {
    for (int i = tid; i < npix; i += HE_THREADS) atomicAdd(&bins[B.index(pix[i])], 1u);
  } else {
    for_pixels(im, npix, [&](int i, T v) { atomicAdd(&bins[B.index(v)], 1u); });
  }
  __syncthreads();
  for (int b = tid; b < nb; b += HE_THREADS)  // density: n / db / n.sum(), db = np.diff(edges) in T
    cdf[b] = ((double)bins[b] / (double)(B.edge(b + 1) - B.edge(b))) / (double)npix;
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

  // read 2: np.interp(v, edges[:-1], cdf) in fp64
  const double e_first = (double)B.edge(0), e_last = (double)B.edge(nb - 1);
  const double scale = (double)nb / (double)B.denom;
  auto interp = [&](int i, T vt) {
    const double v = (double)vt;
    double r;
    if (!(v > e_first)) {  // (also a NaN)
      r = cdf[0];
    } else if (v >= e_last) {
      r = cdf[nb - 1];
    } else {  // e_first < v < e_last: nb >= 2; the interval j in [0, nb - 2] with edge(j) <= v < edge(j + 1)
      double f = (v - e_first) * scale;
      f = f >= 0.0 ? f : 0.0;
      f = f <= (double)(nb - 2) ? f : (double)(nb - 2);
      int j = (int)f;
      while (j > 0 && v < (double)B.edge(j)) --j;
      while (j < nb - 2 && v >= (double)B.edge(j + 1)) ++j;
      const double e0 = (double)B.edge(j), e1 = (double)B.edge(j + 1);
      r = ((cdf[j + 1] - cdf[j]) / (e1 - e0)) * (v - e0) + cdf[j];
    }
    o[i] = r;
  };
  if (keep) {
    for (int i = tid; i < npix; i += HE_THREADS) interp(i, pix[i]);
  } else {
    for_pixels(im, npix, interp);
  }
}

}  // namespace preprocf
}  // namespace ofr

using namespace ofr;
using namespace ofr::preprocf;

static int tt_plan(const char* who, int pixel_bytes, int64_t n, int H, int W, double alpha, double tau, double gamma,
                   double sigma0, double sigma1, Args& a) {
  const std::string w(who);
  OFR_CHECK_ARG(pixel_bytes == 4 || pixel_bytes == 8, w + ": pixel_bytes must be 4 (float32) or 8 (float64)");
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

extern "C" size_t ofr_tantriggs_workspace_bytes_f(int64_t n, int H, int W, double sigma0, double sigma1) {
  Args a;
  if (tt_plan("ofr_tantriggs_workspace_bytes_f", 4, n, H, W, 1.0, 1.0, 1.0, sigma0, sigma1, a) != OFR_OK) return 0;
  return a.nstrips == 1 ? 0 : (size_t)2 * n * a.nstrips * sizeof(double);
}

template <typename T>
static int tt_launch(hipStream_t st, const T* imgs, int64_t n, const Args& a, float* out, double* ws1) {
  static bool attr = false;
  if (!attr) {
    hipError_t e =
        hipFuncSetAttribute((const void*)tantriggs_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(tantriggs_kernel)");
    attr = true;
  }
  const bool strips = a.nstrips > 1;
  const size_t lds = tt_lds(a.SR, a.W, a.R);
  const int64_t npix = (int64_t)a.H * a.W;
  double* ws2 = ws1 ? ws1 + n * a.nstrips : nullptr;
  for (int64_t done = 0; done < n; done += 65535) {
    const int64_t chunk = std::min<int64_t>(n - done, 65535);
    const dim3 grid((unsigned)a.nstrips, (unsigned)chunk);
    double* w1 = strips ? ws1 + done * a.nstrips : nullptr;
    double* w2 = strips ? ws2 + done * a.nstrips : nullptr;
    hipLaunchKernelGGL(tantriggs_kernel<T>, grid, dim3(THREADS), lds, st, imgs + done * npix, a, out + done * npix, w1);
    OFR_LAUNCH_CHECK("tantriggs_kernel");
    if (!strips) continue;
    for (int phase = 0; phase < 2; ++phase) {
      hipLaunchKernelGGL(tantriggs_finish_kernel, grid, dim3(THREADS), 0, st, a, phase, out + done * npix, w1, w2);
      OFR_LAUNCH_CHECK("tantriggs_finish_kernel");
    }
  }
  return OFR_OK;
}

extern "C" int ofr_tantriggs_f32_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W,
                                   double alpha, double tau, double gamma, double sigma0, double sigma1, float* out,
                                   void* workspace, size_t workspace_bytes) {
  Args a;
  int rc = tt_plan("ofr_tantriggs_f32_f", pixel_bytes, n, H, W, alpha, tau, gamma, sigma0, sigma1, a);
  if (rc) return rc;
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs && out, "ofr_tantriggs_f32_f: null pointer");
  OFR_CHECK_ARG((uintptr_t)imgs % (uintptr_t)pixel_bytes == 0 && (uintptr_t)out % 4 == 0,
                "ofr_tantriggs_f32_f: images must be aligned to their pixels");
  const bool strips = a.nstrips > 1;
  const size_t need = strips ? (size_t)2 * n * a.nstrips * sizeof(double) : 0;
  OFR_CHECK_ARG(!strips || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
                "ofr_tantriggs_f32_f: workspace too small (ofr_tantriggs_workspace_bytes_f)");
  if (pixel_bytes == 4) return tt_launch((hipStream_t)stream, (const float*)imgs, n, a, out, (double*)workspace);
  return tt_launch((hipStream_t)stream, (const double*)imgs, n, a, out, (double*)workspace);
}

template <typename T>
static int he_launch(hipStream_t st, const T* imgs, int64_t n, int npix, int num_bins, double* out) {
  static bool attr = false;
  if (!attr) {
    hipError_t e =
        hipFuncSetAttribute((const void*)histeq_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(histeq_kernel)");
    attr = true;
  }
  const size_t fixed = (size_t)num_bins * 8 + HE_FIXED + (size_t)((num_bins + 1) & ~1) * 4;
  const int keep = fixed + (size_t)npix * sizeof(T) <= (size_t)LDS_MAX;
  const size_t lds = fixed + (keep ? (size_t)npix * sizeof(T) : 0);
  hipLaunchKernelGGL(histeq_kernel<T>, dim3((unsigned)n), dim3(HE_THREADS), lds, st, imgs, npix, num_bins, keep, out);
  OFR_LAUNCH_CHECK("histeq_kernel");
  return OFR_OK;
}

extern "C" int ofr_histeq_f64_f(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W,
                                int num_bins, double* out) {
  OFR_CHECK_ARG(pixel_bytes == 4 || pixel_bytes == 8, "ofr_histeq_f64_f: pixel_bytes must be 4 (float32) or 8 (float64)");
  OFR_CHECK_ARG(n >= 0 && H >= 1 && W >= 1, "ofr_histeq_f64_f: bad sizes");
  OFR_CHECK_ARG(num_bins >= 1 && num_bins <= HE_MAXBINS, "ofr_histeq_f64_f: num_bins must be 1..4096");
  OFR_CHECK_ARG(n <= 0x7fffffffLL, "ofr_histeq_f64_f: too many images");
  if (n == 0) return OFR_OK;
  OFR_CHECK_ARG(imgs && out, "ofr_histeq_f64_f: null pointer");
  OFR_CHECK_ARG((uintptr_t)imgs % (uintptr_t)pixel_bytes == 0 && (uintptr_t)out % 8 == 0,
                "ofr_histeq_f64_f: images must be aligned to their pixels");
  const int64_t npix = (int64_t)H * W;
  OFR_CHECK_ARG(npix <= 0x7fffffffLL / 8, "ofr_histeq_f64_f: image too large");
  if (pixel_bytes == 4) return he_launch((hipStream_t)stream, (const float*)imgs, n, (int)npix, num_bins, out);
  return he_launch((hipStream_t)stream, (const double*)imgs, n, (int)npix, num_bins, out);
}
