// VarLBP (reference lbp.py:140-208): the variance of the P interpolated samples on the circle, and its
// per-cell density histograms (feature.py:286-302), on gfx950, bit-exact against numpy 2.x.
//
// Semantics.  Geometry is ExtendedLBP's (ofr_lbp_geom.h).  Per code pixel, all in fp64 without
// contraction, for point i = 0..P-1:
//     N = w1*X; N += w2*X; N += w3*X; N += w4*X          (exact-zero weights dropped on the host)
//     delta = N - mean;  mean = mean + delta / (i+1);  m2 = m2 + delta * (N - mean)
// and the value is m2 / (P-1).  Every `/` is the IEEE fp64 division (the compiler's v_div_scale /
// v_div_fmas / v_div_fixup sequence; no reciprocal multiply, no fast-math), so the image equals the
// reference's bit for bit.  uint8, float32 and float64 pixels are converted exactly to fp64.
// Histogram of one cell = np.histogram(v, bins=2^P, range=(0, 2^P), density=True): v counts when
// 0 <= v <= 2^P (NaN fails both compares), its bin is min((int)v, 2^P - 1) (the edges are the integers,
// v / 2^P * 2^P is exact), and the density is count / total with total the cell's IN-RANGE count -- a
// per-cell denominator, 0/0 = NaN where nothing is in range.  The kernels return the integer counts and
// the totals; the division is ofr_hist_density_f32's (fp32 rows for the searches) or the host's (fp64).
//
// Design.  The band machinery of ofr_lbp_float.hip (ofr_lbp_band.h) carries over; what is new is
// the lane's arithmetic, the binning rule and the totals.
// * A 1024-thread workgroup owns a band of one image: `rows` cell rows (histogram) or `rows` code rows
//   (variance image).  It stages the band's pixel rows into LDS as fp64 behind the u32 counters; the
//   pixel type (1, 4 or 8 bytes) matters there and nowhere else.
// * rows (histogram): the largest whose counters + plane fit 80 KiB (two workgroups per CU), else 160 KiB,
//   evened out over the bands.  rows (variance image): about one code pixel per lane (1024 / dx), so a
//   batch of a few faces still fills the device; the by-1 halo rows are staged twice.
// * Lanes: column i % width of strip i / width, as in the float kernels.  A lane keeps mean and m2 in
//   registers through the P points, then either stores the value or does ONE LDS integer atomic when
//   the value is in range.
// * Radius 1, 8 neighbours: the lane walks its column with the 3 x 3 block in nine fp64 registers (three
//   LDS reads per pixel); the eight Welford steps are straight-line code with constant divisors
//   (1, 2, 4, 8 become exact multiplies, the others stay divisions).  Generic: the points' terms are read
//   from the plane, offsets and weights are kernel arguments.
// * Totals: after the band's barrier, wave w sums the counters of cells w, w + 16, ... (64 lanes stride
//   the 2^P counters, xor-shuffle reduction) and lane 0 writes the int32 total; the counters leave
//   packed as in the float kernels.
// * Global form (not even one cell row fits LDS: gc * 2^P counters above 160 KiB, or very wide images;
//   for the variance image: by rows of W pixels above 160 KiB): pixels through L2, counters as packed
//   atomics on a zeroed destination, then totals_kernel sums each cell with one wave.
#include "ofr_common.h"
#include "ofr_lbp_band.h"
#include "ofr_lbp_geom.h"

#pragma clang fp contract(off)

namespace ofr {
namespace varlbp {

using lbpf::flush_band;
using lbpf::LDS_HALF;
using lbpf::LDS_MAX;
using lbpf::stage_plane;
using lbpf::THREADS;

enum { FORM_GENERIC = 0, FORM_R1P8 = 1 };

struct Band {
  int W;         // image row pitch = plane row pitch
  int img_rows;  // H
  int halo;      // by - 1: pixel rows below the last code row
  int dy, dx;    // code image
  int gr, gc, py, px;
  int rows;      // cell rows (histogram) or code rows (variance image) per band
  int nbands;
  int nb_log2;
  int count_bytes;
  int pixel_bytes;
};

// one Welford step (lbp.py:196-198)
__device__ __forceinline__ void welford(double N, double n, double& mean, double& m2) {
  const double delta = N - mean;
  const double q = delta / n;
  mean = mean + q;
  const double r = N - mean;
  const double prod = delta * r;
  m2 = m2 + prod;
}

// the bin of a value, -1 when np.histogram drops it
__device__ __forceinline__ int bin_of(double v, int nb) {
  if (!(v >= 0.0 && v <= (double)nb)) return -1;
  return min((int)v, nb - 1);
}

// the r = 1, P = 8 value of the 3 x 3 block b (row-major); N as in ofr_lbp_float.hip
__device__ __forceinline__ double var_r1p8(const R1P8& k, double b00, double b01, double b02, double b10, double b11,
                                           double b12, double b20, double b21, double b22) {
  double mean = 0.0, m2 = 0.0, N;
  N = k.w[0][0] * b12;
  welford(N, 1.0, mean, m2);
  N = k.w[1][0] * b01; N = N + k.w[1][1] * b02; N = N + k.w[1][2] * b11; N = N + k.w[1][3] * b12;
  welford(N, 2.0, mean, m2);
  N = k.w[2][0] * b01;
  welford(N, 3.0, mean, m2);
  N = k.w[3][0] * b00; N = N + k.w[3][1] * b01; N = N + k.w[3][2] * b10; N = N + k.w[3][3] * b11;
  welford(N, 4.0, mean, m2);
  N = k.w[4][0] * b00; N = N + k.w[4][2] * b10;
  welford(N, 5.0, mean, m2);
  N = k.w[5][0] * b10; N = N + k.w[5][1] * b11; N = N + k.w[5][2] * b20; N = N + k.w[5][3] * b21;
  welford(N, 6.0, mean, m2);
  N = k.w[6][0] * b20; N = N + k.w[6][1] * b21;
  welford(N, 7.0, mean, m2);
  N = k.w[7][0] * b11; N = N + k.w[7][1] * b12; N = N + k.w[7][2] * b21; N = N + k.w[7][3] * b22;
  welford(N, 8.0, mean, m2);
  return m2 / 7.0;
}

// generic geometry; blk = the code pixel's block origin, pixels of type T (fp64 in LDS, or the image's own)
template <typename T>
__device__ __forceinline__ double var_generic(const T* __restrict__ blk, const LbpGeom& g) {
  double mean = 0.0, m2 = 0.0;
  for (int i = 0; i < g.P; ++i) {
    double N = g.tw[i][0] * (double)blk[g.toff[i][0]];
    for (int t = 1; t < g.nterm[i]; ++t) {  // lbp.py:191-194 order, no contraction
      const double prod = g.tw[i][t] * (double)blk[g.toff[i][t]];
      N = N + prod;
    }
    welford(N, (double)(i + 1), mean, m2);
  }
  return m2 / (double)(g.P - 1);
}

template <int FORM, bool HIST>
__global__ void __launch_bounds__(THREADS) band_kernel(const void* __restrict__ imgs, LbpGeom g, Band a, R1P8 k,
                                                       void* __restrict__ out, int32_t* __restrict__ totals) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const int64_t img = blockIdx.x / a.nbands;
  const int band = blockIdx.x - (int)img * a.nbands;
  const int nb = 1 << a.nb_log2;
  const int W = a.W;
  int r0, hpx, wpx, ncell = 0;  // first code row, code rows, code columns, cells of the band
  double* im;
  if constexpr (HIST) {
    const int cr0 = band * a.rows, cr1 = min(a.gr, cr0 + a.rows);
    r0 = cr0 * a.py;
    hpx = (cr1 - cr0) * a.py;
    wpx = a.gc * a.px;
    ncell = (cr1 - cr0) * a.gc;
    im = reinterpret_cast<double*>(hist + a.rows * a.gc * nb);  // 16-byte aligned: 2^P >= 4 counters per cell
    for (int i = threadIdx.x; i < ncell * nb; i += THREADS) hist[i] = 0;
  } else {
    r0 = band * a.rows;
    hpx = min(a.rows, a.dy - r0);
    wpx = a.dx;
    im = reinterpret_cast<double*>(hist);
  }
  {
    const int64_t first = (img * a.img_rows + r0) * W;  // the band's first pixel
    const int count = (hpx + a.halo) * W;
    if (a.pixel_bytes == 1) stage_plane(reinterpret_cast<const uint8_t*>(imgs) + first, im, count);
    else if (a.pixel_bytes == 4) stage_plane(reinterpret_cast<const float*>(imgs) + first, im, count);
    else stage_plane(reinterpret_cast<const double*>(imgs) + first, im, count);
  }
  __syncthreads();
  double* vals = HIST ? nullptr : reinterpret_cast<double*>(out) + (img * a.dy + r0) * (int64_t)a.dx;
  const int nstrips = max(1, min(hpx, THREADS / wpx));
  const int srows = (hpx + nstrips - 1) / nstrips;
  for (int item = threadIdx.x; item < nstrips * wpx; item += THREADS) {
    const int s = item / wpx, x = item - s * wpx;
    const int ya = s * srows, yb = min(hpx, ya + srows);
    if (ya >= yb) continue;
    int cell0 = 0, ry = 0;  // the lane's cell and the row inside it
    if constexpr (HIST) {
      const int cyc = ya / a.py;
      ry = ya - cyc * a.py;
      cell0 = cyc * a.gc + x / a.px;
    }
    const double* col = im + x;
    double b00, b01, b02, b10, b11, b12;
    if constexpr (FORM == FORM_R1P8) {
      b00 = col[ya * W], b01 = col[ya * W + 1], b02 = col[ya * W + 2];
      b10 = col[(ya + 1) * W], b11 = col[(ya + 1) * W + 1], b12 = col[(ya + 1) * W + 2];
    }
    for (int y = ya; y < yb; ++y) {
      double v;
      if constexpr (FORM == FORM_R1P8) {
        const double* r2 = col + (y + 2) * W;
        const double b20 = r2[0], b21 = r2[1], b22 = r2[2];
        v = var_r1p8(k, b00, b01, b02, b10, b11, b12, b20, b21, b22);
        b00 = b10; b01 = b11; b02 = b12;
        b10 = b20; b11 = b21; b12 = b22;
      } else {
        v = var_generic(col + y * W, g);
      }
      if constexpr (HIST) {
        const int b = bin_of(v, nb);
        if (b >= 0) atomicAdd(&hist[cell0 * nb + b], 1u);
        if (++ry == a.py) {
          ry = 0;
          cell0 += a.gc;
        }
      } else {
        vals[(int64_t)y * a.dx + x] = v;
      }
    }
  }
  if constexpr (HIST) {
    __syncthreads();
    const int64_t cell_base = img * (int64_t)a.gr * a.gc + (int64_t)band * a.rows * a.gc;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c = wave; c < ncell; c += THREADS / 64) {  // wave-uniform: every lane takes part in the shuffles
      uint32_t sum = 0;
      for (int j = lane; j < nb; j += 64) sum += hist[c * nb + j];
      for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
      if (lane == 0) totals[cell_base + c] = (int32_t)sum;
    }
    flush_band(hist, ncell * nb, out, cell_base * nb, a.count_bytes, true);
  }
}

// ---- global form ---------------------------------------------------------------------------------------
struct Global {
  int hist;  // 0: variance image
  int gr, gc, py, px, nb_log2, count_bytes;
};

template <typename T>
__global__ void __launch_bounds__(256) global_kernel(const T* __restrict__ imgs, LbpGeom g, Global a,
                                                     void* __restrict__ out) {
  const int64_t img = blockIdx.y;
  const T* im = imgs + img * (int64_t)g.H * g.W;
  const int npx = g.dy * g.dx;
  const int nb = 1 << a.nb_log2;
  uint32_t* gcounts = reinterpret_cast<uint32_t*>((uint8_t*)out + img * (int64_t)a.gr * a.gc * nb * a.count_bytes);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += gridDim.x * blockDim.x) {
    const int y = p / g.dx, x = p - y * g.dx;
    if (a.hist && !(y < a.gr * a.py && x < a.gc * a.px)) continue;
    const double v = var_generic(im + (int64_t)y * g.W + x, g);
    if (!a.hist) {
      reinterpret_cast<double*>(out)[img * npx + p] = v;
      continue;
    }
    const int b = bin_of(v, nb);
    if (b < 0) continue;
    // the word of the image's packed destination that holds the counter, and its unit there (no byte or
    // half ever carries: a counter ends at most at the cell's pixel count)
    const int64_t idx = (int64_t)((y / a.py) * a.gc + x / a.px) * nb + b;
    if (a.count_bytes == 1) atomicAdd(gcounts + (idx >> 2), 1u << (8 * (int)(idx & 3)));
    else if (a.count_bytes == 2) atomicAdd(gcounts + (idx >> 1), 1u << (16 * (int)(idx & 1)));
    else atomicAdd(gcounts + idx, 1u);
  }
}

__global__ void __launch_bounds__(256) zero_kernel(uint32_t* __restrict__ p, int64_t nwords) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
}

// counts [ncells][2^P] of cb bytes -> totals [ncells]: one wave per cell
__global__ void __launch_bounds__(256) totals_kernel(const void* __restrict__ counts, int cb, int nb_log2,
                                                     int64_t ncells, int32_t* __restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const int64_t nb = 1LL << nb_log2;
  for (int64_t c = blockIdx.x * 4LL + (threadIdx.x >> 6); c < ncells; c += gridDim.x * 4LL) {
    uint32_t sum = 0;
    for (int64_t j = c * nb + lane; j < (c + 1) * nb; j += 64)
      sum += cb == 1 ? ((const uint8_t*)counts)[j] : cb == 2 ? ((const uint16_t*)counts)[j] : ((const uint32_t*)counts)[j];
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) totals[c] = (int32_t)sum;
  }
}

// counts [n][cells][bins] + totals [n][cells] -> fp32 [n][ld]: four columns per thread, one 16-byte store
__global__ void __launch_bounds__(256) density_kernel(const void* __restrict__ counts, int cb,
                                                      const int32_t* __restrict__ totals, int64_t n, int cells,
                                                      int bins, float* __restrict__ out, int ld) {
  const int64_t nbins = (int64_t)cells * bins;
  const int q = ld / 4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n * q; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / q;
    const int j0 = 4 * (int)(i - r * q);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      if (j < nbins) {
        const int64_t at = r * nbins + j;
        const uint32_t c = cb == 1 ? ((const uint8_t*)counts)[at]
                                   : cb == 2 ? ((const uint16_t*)counts)[at] : ((const uint32_t*)counts)[at];
        const double t = (double)totals[r * cells + j / bins];
        v[e] = (float)((double)c / t);  // 0 / 0 = NaN: an empty cell, as in the reference
      } else {
        v[e] = 0.0f;
      }
    }
    reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ---- host side -----------------------------------------------------------------------------------------
static int check_images(const std::string& w, const void* imgs, int pixel_bytes, int64_t n, int H, int W) {
  if (n < 0 || H < 1 || W < 1) return fail(OFR_E_INVALID, w + ": bad sizes");
  if (pixel_bytes != 1 && pixel_bytes != 4 && pixel_bytes != 8)
    return fail(OFR_E_INVALID, w + ": pixel_bytes must be 1 (uint8), 4 (float32) or 8 (float64)");
  if ((int64_t)H * W > 0x7fffffffLL / 2) return fail(OFR_E_UNSUPPORTED, w + ": image too large");
  if ((uintptr_t)imgs % (uintptr_t)pixel_bytes) return fail(OFR_E_INVALID, w + ": images must be aligned to their pixels");
  return OFR_OK;
}

static int check_geom(const std::string& w, LbpGeom& g, int H, int W, int P, const int32_t* offs, const double* wts,
                      int oy, int ox, int by, int bx) {
  if (P < 2) return fail(OFR_E_UNSUPPORTED, w + ": neighbors must be >= 2 (the variance divides by neighbors - 1)");
  if (by < 1 || bx < 1) return fail(OFR_E_INVALID, w + ": bad block size");
  return make_geom(g, H, W, P, offs, wts, oy, ox, by, bx);
}

static int launch_global(hipStream_t st, const void* imgs, int pixel_bytes, int64_t n, const LbpGeom& g,
                         const Global& a, void* out, size_t img_out_bytes) {
  const int npx = g.dy * g.dx;
  const unsigned gx = (unsigned)std::min<int64_t>(cdiv(npx, 256), 64);
  const int64_t img_bytes = (int64_t)g.H * g.W * pixel_bytes;
  for (int64_t done = 0; done < n; done += 65535) {
    const dim3 grid(gx, (unsigned)std::min<int64_t>(n - done, 65535));
    const void* src = (const char*)imgs + done * img_bytes;
    void* o = (void*)((char*)out + done * (int64_t)img_out_bytes);
    if (pixel_bytes == 1) hipLaunchKernelGGL(global_kernel<uint8_t>, grid, dim3(256), 0, st, (const uint8_t*)src, g, a, o);
    else if (pixel_bytes == 4) hipLaunchKernelGGL(global_kernel<float>, grid, dim3(256), 0, st, (const float*)src, g, a, o);
    else hipLaunchKernelGGL(global_kernel<double>, grid, dim3(256), 0, st, (const double*)src, g, a, o);
    OFR_LAUNCH_CHECK("varlbp global_kernel");
  }
  return OFR_OK;
}

template <int FORM, bool HIST>
static int launch_band(hipStream_t st, const void* imgs, int64_t n, const LbpGeom& g, const Band& a, const R1P8& k,
                       size_t lds, void* out, int32_t* totals) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)band_kernel<FORM, HIST>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       LDS_MAX);
    if (e != hipSuccess) return hip_status(e, "hipFuncSetAttribute(varlbp band_kernel)");
    attr = true;
  }
  hipLaunchKernelGGL((band_kernel<FORM, HIST>), dim3((unsigned)(n * a.nbands)), dim3(THREADS), lds, st, imgs, g, a, k,
                     out, totals);
  OFR_LAUNCH_CHECK("varlbp band_kernel");
  return OFR_OK;
}

static int zero_words(hipStream_t st, void* p, int64_t nwords) {
  if (nwords == 0) return OFR_OK;
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nwords, 256), 4096)), dim3(256), 0, st,
                     (uint32_t*)p, nwords);
  OFR_LAUNCH_CHECK("varlbp zero_kernel");
  return OFR_OK;
}

}  // namespace varlbp
}  // namespace ofr

using namespace ofr;
using namespace ofr::varlbp;

extern "C" int ofr_varlbp_values(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int P,
                                 const int32_t* offs_host, const double* w_host, int oy, int ox, int by, int bx,
                                 double* values) {
  int rc = check_images("ofr_varlbp_values", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  LbpGeom g;
  rc = check_geom("ofr_varlbp_values", g, H, W, P, offs_host, w_host, oy, ox, by, bx);
  if (rc) return rc;
  if (n == 0 || g.dy <= 0 || g.dx <= 0) return OFR_OK;
  if (!imgs || !values) return fail(OFR_E_INVALID, "ofr_varlbp_values: null pointer");
  OFR_CHECK_ARG((uintptr_t)values % 8 == 0, "ofr_varlbp_values: values must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // code rows per band: about one code pixel per lane, inside the LDS budgets
  const int64_t row_px = (int64_t)W * 8, halo_px = (int64_t)(by - 1) * row_px;
  auto fit = [&](int64_t budget) { return (budget - halo_px) / row_px; };
  int64_t rows = fit(LDS_HALF);
  if (rows < 1) rows = fit(LDS_MAX);
  rows = std::min<int64_t>(std::min<int64_t>(rows, g.dy), std::max<int64_t>(1, THREADS / g.dx));
  if (rows >= 1 && n * cdiv(g.dy, rows) <= 0x7fffffffLL) {
    Band a = {};
    a.W = W;
    a.img_rows = H;
    a.halo = by - 1;
    a.dy = g.dy;
    a.dx = g.dx;
    a.nbands = (int)cdiv(g.dy, rows);
    a.rows = (int)cdiv(g.dy, a.nbands);
    a.pixel_bytes = pixel_bytes;
    const size_t lds = (size_t)(a.rows * row_px + halo_px);
    R1P8 k = {};
    if (!lbp_generic_forced() && r1p8_match(P, offs_host, w_host, oy, ox, by, bx, k))
      return launch_band<FORM_R1P8, false>(st, imgs, n, g, a, k, lds, values, nullptr);
    return launch_band<FORM_GENERIC, false>(st, imgs, n, g, a, k, lds, values, nullptr);
  }
  Global a = {};
  a.gr = a.gc = a.py = a.px = 1;
  a.count_bytes = 1;
  return launch_global(st, imgs, pixel_bytes, n, g, a, values, (size_t)g.dy * g.dx * 8);
}

extern "C" int ofr_varlbp_hist(void* stream, const void* imgs, int pixel_bytes, int64_t n, int H, int W, int P,
                               const int32_t* offs_host, const double* w_host, int oy, int ox, int by, int bx, int gr,
                               int gc, void* counts, int count_bytes, int32_t* totals) {
  int rc = check_images("ofr_varlbp_hist", imgs, pixel_bytes, n, H, W);
  if (rc) return rc;
  OFR_CHECK_ARG(gr >= 1 && gc >= 1, "ofr_varlbp_hist: bad grid");
  OFR_CHECK_ARG(count_bytes == 1 || count_bytes == 2 || count_bytes == 4, "ofr_varlbp_hist: count_bytes must be 1, 2 or 4");
  if (P > 15) return fail(OFR_E_UNSUPPORTED, "ofr_varlbp_hist: neighbors must be <= 15 for the histogram");
  LbpGeom g;
  rc = check_geom("ofr_varlbp_hist", g, H, W, P, offs_host, w_host, oy, ox, by, bx);
  if (rc) return rc;
  const int py = g.dy > 0 ? g.dy / gr : 0, px = g.dx > 0 ? g.dx / gc : 0;
  const int64_t cell_px = (int64_t)py * px;
  if (count_bytes == 1) OFR_CHECK_ARG(cell_px <= 255, "ofr_varlbp_hist: cell too large for 1-byte counts");
  if (count_bytes == 2) OFR_CHECK_ARG(cell_px <= 65535, "ofr_varlbp_hist: cell too large for 2-byte counts");
  const int64_t nb = 1LL << P, ncells = n * gr * gc;
  OFR_CHECK_ARG((int64_t)gr * gc * nb <= 0x7fffffffLL, "ofr_varlbp_hist: too many counters per image");
  if (n == 0) return OFR_OK;
  if (!imgs || !counts || !totals) return fail(OFR_E_INVALID, "ofr_varlbp_hist: null pointer");
  OFR_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)totals & 3) == 0,
                "ofr_varlbp_hist: counts and totals must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t img_counts = (int64_t)gr * gc * nb * count_bytes;  // a multiple of 4: 2^P >= 4
  if (cell_px == 0) {  // empty cells: all counts and totals zero (the reference's histogram is then NaN)
    rc = zero_words(st, counts, n * (img_counts / 4));
    return rc ? rc : zero_words(st, totals, ncells);
  }
  // cell rows per band: counters + fp64 plane of the band's pixel rows
  const int64_t row_cnt = (int64_t)gc * nb * 4, row_px = (int64_t)py * W * 8, halo_px = (int64_t)(by - 1) * W * 8;
  auto fit = [&](int64_t budget) { return std::min<int64_t>(gr, (budget - halo_px) / (row_cnt + row_px)); };
  int64_t rows = fit(LDS_HALF);
  if (rows < 1) rows = fit(LDS_MAX);
  if (rows >= 1 && n * cdiv(gr, rows) <= 0x7fffffffLL) {
    Band a = {};
    a.W = W;
    a.img_rows = H;
    a.halo = by - 1;
    a.dy = g.dy;
    a.dx = g.dx;
    a.gr = gr;
    a.gc = gc;
    a.py = py;
    a.px = px;
    a.nbands = (int)cdiv(gr, rows);
    a.rows = (int)cdiv(gr, a.nbands);
    a.nb_log2 = P;
    a.count_bytes = count_bytes;
    a.pixel_bytes = pixel_bytes;
    const size_t lds = (size_t)(a.rows * (row_cnt + row_px) + halo_px);
    R1P8 k = {};
    if (!lbp_generic_forced() && r1p8_match(P, offs_host, w_host, oy, ox, by, bx, k))
      return launch_band<FORM_R1P8, true>(st, imgs, n, g, a, k, lds, counts, totals);
    return launch_band<FORM_GENERIC, true>(st, imgs, n, g, a, k, lds, counts, totals);
  }
  rc = zero_words(st, counts, n * (img_counts / 4));
  if (rc) return rc;
  Global a = {};
  a.hist = 1;
  a.gr = gr;
  a.gc = gc;
  a.py = py;
  a.px = px;
  a.nb_log2 = P;
  a.count_bytes = count_bytes;
  rc = launch_global(st, imgs, pixel_bytes, n, g, a, counts, (size_t)img_counts);
  if (rc) return rc;
  hipLaunchKernelGGL(totals_kernel, dim3((unsigned)std::min<int64_t>(cdiv(ncells, 4), 65536)), dim3(256), 0, st, counts,
                     count_bytes, P, ncells, totals);
  OFR_LAUNCH_CHECK("varlbp totals_kernel");
  return OFR_OK;
}

extern "C" int ofr_hist_density_f32(void* stream, const void* counts, int count_bytes, const int32_t* totals,
                                    int64_t n, int cells, int bins, float* out, int64_t ld) {
  OFR_CHECK_ARG(n >= 0 && cells >= 1 && bins >= 1, "ofr_hist_density_f32: bad sizes");
  OFR_CHECK_ARG(count_bytes == 1 || count_bytes == 2 || count_bytes == 4,
                "ofr_hist_density_f32: count_bytes must be 1, 2 or 4");
  const int64_t nbins = (int64_t)cells * bins;
  OFR_CHECK_ARG(nbins <= 0x7fffffffLL - 3 && ld == round_up(nbins, 4),
                "ofr_hist_density_f32: ld must be cells * bins rounded up to 4");
  if (n == 0) return OFR_OK;
  if (!counts || !totals || !out) return fail(OFR_E_INVALID, "ofr_hist_density_f32: null pointer");
  OFR_CHECK_ARG((uintptr_t)counts % (uintptr_t)count_bytes == 0 && ((uintptr_t)totals & 3) == 0 &&
                    ((uintptr_t)out & 15) == 0,
                "ofr_hist_density_f32: counts / totals must be aligned to their elements, out to 16 bytes");
  const int64_t items = n * (ld / 4);
  hipLaunchKernelGGL(density_kernel, dim3((unsigned)std::min<int64_t>(cdiv(items, 256), 65536)), dim3(256), 0,
                     (hipStream_t)stream, counts, count_bytes, totals, n, cells, bins, out, (int)ld);
  OFR_LAUNCH_CHECK("hist density_kernel");
  return OFR_OK;
}
