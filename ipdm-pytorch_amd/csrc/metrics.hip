// libipdm_hip.so -- the five image-quality metrics of metric_calculate (Utils/train_test_utils.py:789-806) as HIP kernels.
//
// Replaces, per scored image, skimage's peak_signal_noise_ratio / structural_similarity, piq's vif_p / fsim and Utils/NQM.py
// as ipdm-pytorch_amd/evaluate.py restates them (compare_psnr, compare_ssim, vif_p, NQM, fsim).  Everything is float64:
// the work is a few dozen 2-D FFTs and a handful of small convolutions per image, nothing beside a UNet forward, and the gate
// (tests/test_gpu_metrics.py) compares against a float64 evaluation.
//   * every reduction is per slice, one workgroup, fixed order: a batch is bit-equal to single-slice calls, two calls are
//     bit-equal (the only atomics are integer histogram counts of the radix select);
//   * the 2-D FFT is an in-LDS radix-2 pass over rows, then over groups of columns; twiddles come from a float64 host table;
//   * NQM runs ONE forward transform of ref + i*img and six inverse ones (the band filters are even, so the real and imaginary
//     parts of an inverse transform are the reference's and the image's band); FSIM runs one forward transform of the pair and
//     splits the two spectra by Hermitian symmetry, then eight inverse transforms per orientation.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>
#include "common.h"

using namespace ipdm;

namespace {

constexpr int NACC = 16;          // accumulator slots per slice
enum { A_SSE = 0, A_SSIM = 1, A_VNUM = 2, A_VDEN = 6, A_NQ1 = 10, A_NQ2 = 11, A_FS1 = 12, A_FS2 = 13 };
enum { M_PSNR = 1, M_SSIM = 2, M_FSIM = 4, M_VIF = 8, M_NQM = 16 };
constexpr double kPi = 3.141592653589793;

struct FsimConsts {               // image-independent scalars of _phase_congruency
    double sum_f0sq[4], sum_an2[4], sum_aiaj[4];
    double ln_half, sqrt_half_pi, two_minus_half_pi, k;
};
struct NqmConsts { double ct[6], d[6]; };

}  // namespace

struct ipdm_metrics_plan {
    int H = 0, W = 0, fft_ok = 0, ks = 1, h2 = 0, w2 = 0, nmax = 0;
    std::vector<double> bands;        // [6][H][W], fftshift'ed
    std::vector<double> filt;         // [4 orient][4 scale][h2][w2]
    std::vector<double> tw;           // [nmax/2][2]
    std::vector<double> vifk;         // 17^2 + 9^2 + 5^2 + 3^2
    FsimConsts fc;
    NqmConsts nc;
    double *d_bands = nullptr, *d_filt = nullptr, *d_tw = nullptr, *d_vifk = nullptr;
};

namespace {

bool pow2_in_range(int n) { return n >= 64 && n <= 1024 && (n & (n - 1)) == 0; }
int ilog2(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }

double ctf(double f) { return 1.0 / (200 * (2.6 * (0.0192 + 0.114 * f) * exp(-pow(0.114 * f, 1.1)))); }

// pairwise sum: the plan's scalar tables are sums of 65536 non-negative terms
double pairwise(const double *v, size_t n)
{
    if (n <= 8) { double s = 0; for (size_t i = 0; i < n; ++i) s += v[i]; return s; }
    return pairwise(v, n / 2) + pairwise(v + n / 2, n - n / 2);
}

void build_vif_kernels(std::vector<double> &out)
{
    out.clear();
    for (int scale = 0; scale < 4; ++scale) {
        const int n = (1 << (4 - scale)) + 1;
        const double sigma = n / 5.0;
        std::vector<double> g(n);
        for (int i = 0; i < n; ++i) { double c = (double)i - (n - 1) / 2.0; g[i] = exp(-(c * c) / (2 * sigma * sigma)); }
        std::vector<double> k((size_t)n * n);
        for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) k[(size_t)i * n + j] = g[i] * g[j];
        const double s = pairwise(k.data(), k.size());            // numpy's k.sum() is pairwise too
        for (auto &v : k) out.push_back(v / s);
    }
}
int vif_kernel_offset(int scale) { int o = 0; for (int s = 0; s < scale; ++s) { int n = (1 << (4 - s)) + 1; o += n * n; } return o; }

// NQM's six cosine-log bands (evaluate.NQM / Utils/NQM.py), stored fftshift'ed: the form the spectrum is multiplied with
void build_nqm_bands(ipdm_metrics_plan *p)
{
    const int H = p->H, W = p->W;
    p->bands.assign((size_t)6 * H * W, 0.0);
    const double lo[6] = {1, 1, 2, 4, 8, 16}, hi[6] = {4, 4, 8, 16, 32, 64}, fill[6] = {4, 4, .5, 4, .5, 4};
    const double shift[6] = {kPi, kPi, 0.0, kPi, 0.0, kPi};
    for (int k = 0; k < 6; ++k)
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                const int si = (i + H / 2) % H, sj = (j + W / 2) % W;          // fftshift: out[i] = in[(i + n/2) % n]
                const double xp = -(double)W / 2 + sj, yp = -(double)H / 2 + si;
                double rr = hypot(xp, yp);
                if (k == 0) rr = rr + 2;
                const bool inside = rr >= lo[k] && rr <= hi[k];
                const double v = inside ? rr : fill[k];
                p->bands[((size_t)k * H + i) * W + j] = 0.5 * (1 + cos(kPi * log2(v) - shift[k]));
            }
    for (int k = 1; k < 6; ++k) { p->nc.ct[k] = ctf((double)k); p->nc.d[k] = ctf((double)(1 << k)); }
    p->nc.ct[0] = p->nc.d[0] = 0;
}

// FSIM's lowpass x log-Gabor x angular-spread bank (evaluate._phase_congruency) at the down-sampled size, unshifted (DC at
// [0, 0]), and the three image-independent sums per orientation.  fi = Re(ifft2(f)) sqrt(hw) is the inverse transform of the
// even part fe(k) = (f(k) + f(-k)) / 2, so by Parseval sum(fi_a fi_b) = sum(fe_a fe_b): no host FFT is needed.
void build_fsim_bank(ipdm_metrics_plan *p)
{
    const int h = p->h2, w = p->w2;
    const size_t n = (size_t)h * w;
    p->filt.assign(16 * n, 0.0);
    std::vector<double> radius(n), theta(n), lowpass(n);
    for (int i = 0; i < h; ++i)
        for (int j = 0; j < w; ++j) {
            const double gx = (-(double)h / 2 + (i + h / 2) % h) / h, gy = (-(double)w / 2 + (j + w / 2) % w) / w;   // ifftshift
            const double r = sqrt(gx * gx + gy * gy);
            radius[(size_t)i * w + j] = r;
            theta[(size_t)i * w + j] = atan2(-gy, gx);
            lowpass[(size_t)i * w + j] = 1.0 / (1.0 + pow(r / 0.45, 30.0));
        }
    radius[0] = 1;
    const double ls = log(0.55);
    const double theta_sigma = kPi / (4 * 1.2);
    for (int o = 0; o < 4; ++o) {
        const double ang = o * kPi / 4;
        for (size_t e = 0; e < n; ++e) {
            const double ds = sin(theta[e]) * cos(ang) - cos(theta[e]) * sin(ang);
            const double dc = cos(theta[e]) * cos(ang) + sin(theta[e]) * sin(ang);
            const double a = fabs(atan2(ds, dc));
            const double spread = exp(-(a * a) / (2 * theta_sigma * theta_sigma));
            for (int s = 0; s < 4; ++s) {
                const double f0 = 1.0 / (6 * (double)(1 << s));
                const double lg = log(radius[e] / f0);
                double g = exp(-(lg * lg) / (2 * (ls * ls))) * lowpass[e];
                if (e == 0) g = 0;
                p->filt[((size_t)(o * 4 + s)) * n + e] = spread * g;
            }
        }
        std::vector<double> t(n);
        const double *f0p = &p->filt[(size_t)(o * 4) * n];
        for (size_t e = 0; e < n; ++e) t[e] = f0p[e] * f0p[e];
        p->fc.sum_f0sq[o] = pairwise(t.data(), n);
        std::vector<std::vector<double>> fe(4, std::vector<double>(n));
        for (int s = 0; s < 4; ++s) {
            const double *f = &p->filt[(size_t)(o * 4 + s) * n];
            for (int i = 0; i < h; ++i)
                for (int j = 0; j < w; ++j)
                    fe[s][(size_t)i * w + j] = 0.5 * (f[(size_t)i * w + j] + f[(size_t)((h - i) % h) * w + (w - j) % w]);
        }
        double an2 = 0, aiaj = 0;
        for (int s = 0; s < 4; ++s) {
            for (size_t e = 0; e < n; ++e) t[e] = fe[s][e] * fe[s][e];
            an2 += pairwise(t.data(), n);
        }
        for (int a = 0; a < 3; ++a)
            for (int b = a + 1; b < 4; ++b) {
                for (size_t e = 0; e < n; ++e) t[e] = fe[a][e] * fe[b][e];
                aiaj += pairwise(t.data(), n);
            }
        p->fc.sum_an2[o] = an2;
        p->fc.sum_aiaj[o] = aiaj;
    }
    p->fc.ln_half = log(0.5);
    p->fc.sqrt_half_pi = sqrt(kPi / 2);
    p->fc.two_minus_half_pi = 2 - kPi / 2;
    p->fc.k = 2.0;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ void __launch_bounds__(256) prep_kernel(const float *__restrict__ ref, long ref_stride, const float *__restrict__ img,
                                                   double *__restrict__ R, double *__restrict__ I, long n)
{
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const float v = img[(size_t)b * n + e];
    R[(size_t)b * n + e] = (double)ref[(size_t)b * ref_stride + e];
    I[(size_t)b * n + e] = (v != v) ? 0.5 : (double)v;          // metric_calculate: ld[np.isnan(ld)] = 0.5
}

// acc[b][slot + q] = sum of src[q][b][0..n) -- one workgroup per (q, slice), fixed order
__global__ void __launch_bounds__(1024) reduce_kernel(const double *__restrict__ src, long n, long slice_stride, long q_stride,
                                                      double *__restrict__ acc, int slot)
{
    __shared__ double sh[1024];
    const int b = blockIdx.y, q = blockIdx.x;
    const double *s = src + (size_t)q * q_stride + (size_t)b * slice_stride;
    double v = 0;
    for (long i = threadIdx.x; i < n; i += 1024) v += s[i];
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) acc[(size_t)b * NACC + slot + q] = sh[0];
}

__global__ void __launch_bounds__(256) sqerr_kernel(const double *__restrict__ R, const double *__restrict__ I, double *__restrict__ T, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t o = (size_t)blockIdx.y * n + e;
    const double d = R[o] - I[o];
    T[o] = d * d;
}

// SSIM map on the interior (the cropped border equals the window radius): T[b][(H-10)*(W-10)]
__global__ void __launch_bounds__(256) ssim_kernel(const double *__restrict__ R, const double *__restrict__ I, double *__restrict__ T,
                                                   int H, int W, long t_stride)
{
    const int oh = H - 10, ow = W - 10;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)oh * ow) return;
    const int y = (int)(e / ow), x = (int)(e % ow);
    const double *r = R + (size_t)blockIdx.y * H * W, *q = I + (size_t)blockIdx.y * H * W;
    double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
    for (int i = 0; i < 11; ++i)
        for (int j = 0; j < 11; ++j) {
            const double a = r[(size_t)(y + i) * W + x + j], c = q[(size_t)(y + i) * W + x + j];
            sx += a; sy += c; sxx += a * a; syy += c * c; sxy += a * c;
        }
    const double ux = sx / 121.0, uy = sy / 121.0, uxx = sxx / 121.0, uyy = syy / 121.0, uxy = sxy / 121.0;
    const double cn = 121.0 / 120.0;
    const double vx = cn * (uxx - ux * ux), vy = cn * (uyy - uy * uy), vxy = cn * (uxy - ux * uy);
    const double C1 = (0.01 * 1.0) * (0.01 * 1.0), C2 = (0.03 * 1.0) * (0.03 * 1.0);
    T[(size_t)blockIdx.y * t_stride + e] = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
}

// VIF: valid convolution + factor-2 decimation of both images (dst [oh][ow], oh = ceil((h - n + 1) / 2))
__global__ void __launch_bounds__(256) vif_down_kernel(const double *__restrict__ sx, const double *__restrict__ sy, int h, int w,
                                                       long s_stride, double mult, const double *__restrict__ k, int n,
                                                       double *__restrict__ dx, double *__restrict__ dy, long d_stride)
{
    const int oh = (h - n + 2) / 2, ow = (w - n + 2) / 2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)oh * ow) return;
    const int y = 2 * (int)(e / ow), x = 2 * (int)(e % ow);
    const double *a = sx + (size_t)blockIdx.y * s_stride, *c = sy + (size_t)blockIdx.y * s_stride;
    double ax = 0, ay = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double kv = k[i * n + j];
            ax += kv * (a[(size_t)(y + i) * w + x + j] * mult);
            ay += kv * (c[(size_t)(y + i) * w + x + j] * mult);
        }
    dx[(size_t)blockIdx.y * d_stride + e] = ax;
    dy[(size_t)blockIdx.y * d_stride + e] = ay;
}

// VIF: the per-pixel information terms of one scale (numerator and denominator), output [(h-n+1)*(w-n+1)]
__global__ void __launch_bounds__(256) vif_stats_kernel(const double *__restrict__ sx, const double *__restrict__ sy, int h, int w,
                                                        long s_stride, double mult, const double *__restrict__ k, int n,
                                                        double *__restrict__ Tn, double *__restrict__ Td, long t_stride)
{
    const int oh = h - n + 1, ow = w - n + 1;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)oh * ow) return;
    const int y = (int)(e / ow), x = (int)(e % ow);
    const double *a = sx + (size_t)blockIdx.y * s_stride, *c = sy + (size_t)blockIdx.y * s_stride;
    double mx = 0, my = 0, mxx = 0, myy = 0, mxy = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double kv = k[i * n + j];
            const double u = a[(size_t)(y + i) * w + x + j] * mult, v = c[(size_t)(y + i) * w + x + j] * mult;
            mx += kv * u; my += kv * v; mxx += kv * (u * u); myy += kv * (v * v); mxy += kv * (u * v);
        }
    const double eps = 1e-8, sigma_n_sq = 2.0;
    double sxx = fmax(mxx - mx * mx, 0.0), syy = fmax(myy - my * my, 0.0);
    const double sxy = mxy - mx * my;
    double g = sxy / (sxx + eps);
    double sv = syy - g * sxy;
    if (sxx < eps) { g = 0.0; sv = syy; sxx = 0.0; }
    if (syy < eps) { g = 0.0; sv = 0.0; }
    if (g < 0) { sv = syy; g = 0.0; }
    sv = fmax(sv, eps);
    Tn[(size_t)blockIdx.y * t_stride + e] = log10(1.0 + (g * g) * sxx / (sv + sigma_n_sq));
    Td[(size_t)blockIdx.y * t_stride + e] = log10(1.0 + sxx / sigma_n_sq);
}

// 1-D FFT of length n over L lines per workgroup, in LDS (radix-2, decimation in time).  Image `blockIdx.y` of
// [n_other][n] (rows: a line is a row) or [n][n_other] (COLS: a line is a column, L adjacent columns share the 64-byte
// lines they are read from).  tw[k] = exp(-2 pi i k / (n * tw_stride)).
template <bool COLS>
__global__ void __launch_bounds__(256) fft_kernel(double2 *__restrict__ data, int n, int log2n, int n_other, int L,
                                                  const double2 *__restrict__ tw, int tw_stride, int inverse, double scale)
{
    extern __shared__ double2 s_fft[];
    double2 *img = data + (size_t)blockIdx.y * n * n_other;
    const int l0 = blockIdx.x * L;
    for (int e = threadIdx.x; e < L * n; e += 256) {
        int l, i;
        size_t src;
        if (COLS) { l = e % L; i = e / L; src = (size_t)i * n_other + l0 + l; }
        else { l = e / n; i = e % n; src = (size_t)(l0 + l) * n + i; }
        s_fft[l * n + (int)(__brev((unsigned)i) >> (32 - log2n))] = img[src];
    }
    __syncthreads();
    const int halfn = n >> 1;
    for (int st = 0; st < log2n; ++st) {
        const int half = 1 << st;
        for (int j = threadIdx.x; j < L * halfn; j += 256) {
            const int l = j / halfn, jj = j % halfn;
            const int grp = jj >> st, k = jj & (half - 1);
            const int i0 = l * n + (grp << (st + 1)) + k, i1 = i0 + half;
            double2 w = tw[(size_t)(k << (log2n - 1 - st)) * tw_stride];
            if (inverse) w.y = -w.y;
            const double2 a = s_fft[i0], c = s_fft[i1];
            const double tr = w.x * c.x - w.y * c.y, ti = w.x * c.y + w.y * c.x;
            s_fft[i0] = make_double2(a.x + tr, a.y + ti);
            s_fft[i1] = make_double2(a.x - tr, a.y - ti);
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < L * n; e += 256) {
        int l, i;
        size_t dst;
        if (COLS) { l = e % L; i = e / L; dst = (size_t)i * n_other + l0 + l; }
        else { l = e / n; i = e % n; dst = (size_t)(l0 + l) * n + i; }
        const double2 v = s_fft[l * n + i];
        img[dst] = make_double2(v.x * scale, v.y * scale);
    }
}

__global__ void __launch_bounds__(256) pack_kernel(const double *__restrict__ R, const double *__restrict__ I, double2 *__restrict__ Z, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t o = (size_t)blockIdx.y * n + e;
    Z[o] = make_double2(R[o], I[o]);
}

// C[b][k] = band_k * Z[b]   (grid.z = 6 bands)
__global__ void __launch_bounds__(256) nqm_mult_kernel(const double2 *__restrict__ Z, const double *__restrict__ bands,
                                                       double2 *__restrict__ C, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int b = blockIdx.y, k = blockIdx.z;
    const double g = bands[(size_t)k * n + e];
    const double2 z = Z[(size_t)b * n + e];
    C[((size_t)b * 6 + k) * n + e] = make_double2(g * z.x, g * z.y);
}

// the band recurrence of NQM: contrasts against the running sum, contrast masking, global threshold.  IEEE division and
// comparisons: inf / NaN contrasts compare false exactly as in numpy's np.where masks.
__global__ void __launch_bounds__(256) nqm_point_kernel(const double2 *__restrict__ C, NqmConsts nc, double *__restrict__ T1,
                                                        double *__restrict__ T2, long n)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int b = blockIdx.y;
    double2 v = C[((size_t)b * 6) * n + e];
    double so = v.x, si = v.y, y1 = 0, y2 = 0;
    for (int k = 1; k < 6; ++k) {
        v = C[((size_t)b * 6 + k) * n + e];
        const double bo = v.x, bi = v.y;
        const double c = bo / so, ci = bi / si;
        const double ct = nc.ct[k], d = nc.d[k];
        const double cic = fabs(ci) > 1 ? 1.0 : ci;
        const double Tm = ct * (.86 * ((c / ct) - 1) + .3);
        const double ai = ((fabs(cic - c) - Tm) < 0) ? bo : bi;
        y1 = y1 + ((fabs(c) < d) ? 0.0 : bo);
        y2 = y2 + ((fabs(ci) < d) ? 0.0 : ai);
        so += bo;
        si += bi;
    }
    T1[(size_t)b * n + e] = y1 * y1;
    T2[(size_t)b * n + e] = (y1 - y2) * (y1 - y2);
}

// FSIM: both images on 0..255, ks x ks block means; Z2 = a + i b
__global__ void __launch_bounds__(256) fsim_down_kernel(const double *__restrict__ R, const double *__restrict__ I, int H, int W, int ks,
                                                        int h2, int w2, double *__restrict__ A, double *__restrict__ Bm,
                                                        double2 *__restrict__ Z)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)h2 * w2) return;
    const int y = (int)(e / w2), x = (int)(e % w2);
    const double *r = R + (size_t)blockIdx.y * H * W, *q = I + (size_t)blockIdx.y * H * W;
    double sa = 0, sb = 0;
    for (int i = 0; i < ks; ++i)
        for (int j = 0; j < ks; ++j) {
            sa += r[(size_t)(y * ks + i) * W + x * ks + j] * 255.0;
            sb += q[(size_t)(y * ks + i) * W + x * ks + j] * 255.0;
        }
    sa /= (double)(ks * ks);
    sb /= (double)(ks * ks);
    const size_t o = (size_t)blockIdx.y * h2 * w2 + e;
    A[o] = sa; Bm[o] = sb; Z[o] = make_double2(sa, sb);
}

// C[b][img*4 + s] = filt[o][s] * F_img, the two spectra split out of Z = fft2(a + i b) by Hermitian symmetry (grid.z = 4 scales)
__global__ void __launch_bounds__(256) fsim_mult_kernel(const double2 *__restrict__ Z, const double *__restrict__ filt_o, int h2, int w2,
                                                        double2 *__restrict__ C)
{
    const long n = (long)h2 * w2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int b = blockIdx.y, s = blockIdx.z;
    const int y = (int)(e / w2), x = (int)(e % w2);
    const double2 z = Z[(size_t)b * n + e];
    const double2 m = Z[(size_t)b * n + (size_t)((h2 - y) % h2) * w2 + (w2 - x) % w2];
    const double f = filt_o[(size_t)s * n + e];
    const double far = 0.5 * (z.x + m.x), fai = 0.5 * (z.y - m.y);
    const double fbr = 0.5 * (z.y + m.y), fbi = -0.5 * (z.x - m.x);
    C[((size_t)b * 8 + s) * n + e] = make_double2(f * far, f * fai);
    C[((size_t)b * 8 + 4 + s) * n + e] = make_double2(f * fbr, f * fbi);
}

// per orientation and image (grid.z = 2): amplitude sum, phase-deviation energy, |eo[0]|^2
__global__ void __launch_bounds__(256) fsim_pc_kernel(const double2 *__restrict__ C, long n, double *__restrict__ An, double *__restrict__ En,
                                                      double *__restrict__ E0)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int b = blockIdx.y, im = blockIdx.z;
    double2 v[4];
    double an = 0, se = 0, so = 0;
    for (int s = 0; s < 4; ++s) {
        v[s] = C[((size_t)b * 8 + im * 4 + s) * n + e];
        an += hypot(v[s].x, v[s].y);
        se += v[s].x;
        so += v[s].y;
    }
    const double xen = sqrt(se * se + so * so) + DBL_EPSILON;
    const double me = se / xen, mo = so / xen;
    double en = 0;
    for (int s = 0; s < 4; ++s) en += v[s].x * me + v[s].y * mo - fabs(v[s].x * mo - v[s].y * me);
    const size_t o = ((size_t)b * 2 + im) * n + e;
    const double a0 = hypot(v[0].x, v[0].y);
    An[o] = an; En[o] = en; E0[o] = a0 * a0;
}

// order statistic n/2 - 1 + blockIdx.x of the non-negative doubles of image blockIdx.y: 8-bit radix select on the bit pattern
// (monotonic for values >= +0), one workgroup, integer LDS counts only.  out[img][2].
__global__ void __launch_bounds__(1024) select_kernel(const double *__restrict__ x, long n, double *__restrict__ out)
{
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ unsigned int s_k;
    const double *src = x + (size_t)blockIdx.y * n;
    if (threadIdx.x == 0) { s_prefix = 0ull; s_k = (unsigned int)(n / 2 - 1 + blockIdx.x); }
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const unsigned long long mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (long i = threadIdx.x; i < n; i += 1024) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(src[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(unsigned int)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned int k = s_k, cum = 0;
            int bin = 255;
            for (int i = 0; i < 256; ++i) {
                if (cum + hist[i] > k) { bin = i; break; }
                cum += hist[i];
            }
            s_prefix = prefix | ((unsigned long long)bin << shift);
            s_k = k - cum;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * 2 + blockIdx.x] = __longlong_as_double((long long)s_prefix);
}

// energy_all += max(energy - T, 0), an_all += an  (T from the median of |eo[0]|^2: Rayleigh noise model)
__global__ void __launch_bounds__(256) fsim_acc_kernel(const double *__restrict__ An, const double *__restrict__ En, const double *__restrict__ med,
                                                       FsimConsts fc, int o, long n, double *__restrict__ Eall, double *__restrict__ Aall)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t im = blockIdx.y;                                   // slice * 2 + image
    const double median = (med[im * 2] + med[im * 2 + 1]) / 2;      // np.median of an even count
    const double noise_power = (-median / fc.ln_half) / fc.sum_f0sq[o];
    const double tau = sqrt((2 * noise_power * fc.sum_an2[o] + 4 * noise_power * fc.sum_aiaj[o]) / 2);
    const double t = (tau * fc.sqrt_half_pi + fc.k * sqrt(fc.two_minus_half_pi * (tau * tau))) / 1.7;
    const size_t idx = im * n + e;
    const double ea = o == 0 ? 0.0 : Eall[idx], aa = o == 0 ? 0.0 : Aall[idx];
    Eall[idx] = ea + fmax(En[idx] - t, 0.0);
    Aall[idx] = aa + An[idx];
}

__device__ inline double scharr_mag(const double *a, int h, int w, int y, int x)
{
    auto at = [&](int yy, int xx) -> double { return (yy < 0 || yy >= h || xx < 0 || xx >= w) ? 0.0 : a[(size_t)yy * w + xx]; };
    const double k3 = 3.0 / 16, k10 = 10.0 / 16;
    const double gx = -k3 * at(y - 1, x - 1) + k3 * at(y - 1, x + 1) - k10 * at(y, x - 1) + k10 * at(y, x + 1) - k3 * at(y + 1, x - 1) +
                      k3 * at(y + 1, x + 1);
    const double gy = -k3 * at(y - 1, x - 1) - k10 * at(y - 1, x) - k3 * at(y - 1, x + 1) + k3 * at(y + 1, x - 1) + k10 * at(y + 1, x) +
                      k3 * at(y + 1, x + 1);
    return sqrt(gx * gx + gy * gy);
}

__global__ void __launch_bounds__(256) fsim_final_kernel(const double *__restrict__ A, const double *__restrict__ Bm, const double *__restrict__ Eall,
                                                         const double *__restrict__ Aall, int h2, int w2, double *__restrict__ T1,
                                                         double *__restrict__ T2, long t_stride)
{
    const long n = (long)h2 * w2;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t b = blockIdx.y;
    const int y = (int)(e / w2), x = (int)(e % w2);
    const double eps = DBL_EPSILON;
    const double pa = (Eall[(b * 2) * n + e] + eps) / (Aall[(b * 2) * n + e] + eps);
    const double pb = (Eall[(b * 2 + 1) * n + e] + eps) / (Aall[(b * 2 + 1) * n + e] + eps);
    const double ga = scharr_mag(A + b * n, h2, w2, y, x), gb = scharr_mag(Bm + b * n, h2, w2, y, x);
    const double s_pc = (2 * pa * pb + 0.85) / (pa * pa + pb * pb + 0.85);
    const double s_g = (2 * ga * gb + 160) / (ga * ga + gb * gb + 160);
    const double pm = fmax(pa, pb);
    T1[b * t_stride + e] = s_g * s_pc * pm;
    T2[b * t_stride + e] = pm;
}

__global__ void finalize_kernel(const double *__restrict__ acc, double *__restrict__ out, unsigned mask, double n, double n_ssim)
{
    const int b = blockIdx.x;
    const double *a = acc + (size_t)b * NACC;
    double *o = out + (size_t)b * 5;
    if (mask & M_PSNR) o[0] = 10 * log10((1.0 * 1.0) / (a[A_SSE] / n));
    if (mask & M_SSIM) o[1] = a[A_SSIM] / n_ssim;
    if (mask & M_FSIM) o[2] = a[A_FS1] / a[A_FS2];
    if (mask & M_VIF) {
        double num = 0.0, den = 0.0;
        for (int s = 0; s < 4; ++s) { num += a[A_VNUM + s]; den += a[A_VDEN + s]; }
        o[3] = (num + 1e-8) / (den + 1e-8);
    }
    if (mask & M_NQM) o[4] = 10 * log10(a[A_NQ1] / a[A_NQ2]);
}

// ------------------------------------------------------------------------------------------------ workspace
struct Carve {
    char *base;
    size_t off = 0;
    explicit Carve(void *b) : base((char *)b) {}
    template <typename T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + off) : nullptr;
        off += align_up(count * sizeof(T), 256);
        return p;
    }
};

struct Ws {
    double *acc, *R, *I, *T0, *T1, *P[4], *FA, *FB, *An, *En, *E0, *Eall, *Aall, *med;
    double2 *Z, *C;
};

void vif_dims(int H, int W, int hs[4], int ws[4])
{
    hs[0] = H; ws[0] = W;
    for (int s = 1; s < 4; ++s) { const int n = (1 << (4 - s)) + 1; hs[s] = (hs[s - 1] - n + 2) / 2; ws[s] = (ws[s - 1] - n + 2) / 2; }
}

size_t carve(const ipdm_metrics_plan *p, int B, unsigned mask, void *base, Ws *w)
{
    Carve c(base);
    const size_t n = (size_t)p->H * p->W, n2 = (size_t)p->h2 * p->w2;
    Ws t{};
    t.acc = c.take<double>((size_t)B * NACC);
    t.R = c.take<double>(B * n);
    t.I = c.take<double>(B * n);
    t.T0 = c.take<double>(B * n);
    t.T1 = c.take<double>(B * n);
    if (mask & M_VIF) for (int i = 0; i < 4; ++i) t.P[i] = c.take<double>(B * (n / 4 + 1));
    if (mask & (M_NQM | M_FSIM)) {
        t.Z = c.take<double2>(B * n);
        const size_t cn = std::max((mask & M_NQM) ? 6 * n : 0, (mask & M_FSIM) ? 8 * n2 : 0);
        t.C = c.take<double2>(B * cn);
    }
    if (mask & M_FSIM) {
        t.FA = c.take<double>(B * n2);
        t.FB = c.take<double>(B * n2);
        t.An = c.take<double>(2 * B * n2);
        t.En = c.take<double>(2 * B * n2);
        t.E0 = c.take<double>(2 * B * n2);
        t.Eall = c.take<double>(2 * B * n2);
        t.Aall = c.take<double>(2 * B * n2);
        t.med = c.take<double>((size_t)4 * B);
    }
    if (w) *w = t;
    return c.off;
}

void fft2d(double2 *data, int nimg, int h, int w, const ipdm_metrics_plan *p, int inverse, hipStream_t st)
{
    const double2 *tw = (const double2 *)p->d_tw;
    const int Lr = w <= 512 ? 2 : 1;
    hipLaunchKernelGGL(fft_kernel<false>, dim3(h / Lr, nimg), dim3(256), (size_t)Lr * w * sizeof(double2), st, data, w, ilog2(w), h, Lr, tw,
                       p->nmax / w, inverse, 1.0);
    const int Lc = h <= 512 ? 4 : 2;
    hipLaunchKernelGGL(fft_kernel<true>, dim3(w / Lc, nimg), dim3(256), (size_t)Lc * h * sizeof(double2), st, data, h, ilog2(h), w, Lc, tw,
                       p->nmax / h, inverse, inverse ? 1.0 / ((double)h * w) : 1.0);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ ABI
extern "C" int ipdm_metrics_plan_create(int32_t H, int32_t W, ipdm_metrics_plan **out)
{
    IPDM_REQUIRE(out, "metrics_plan_create: null argument");
    IPDM_REQUIRE(H >= 64 && W >= 64 && H <= 8192 && W <= 8192, "metrics_plan_create: image size %d x %d outside 64 .. 8192", H, W);
    ipdm_metrics_plan *p = new ipdm_metrics_plan();
    p->H = H; p->W = W;
    p->fft_ok = pow2_in_range(H) && pow2_in_range(W);
    const int mn = H < W ? H : W;
    const int ks = (int)nearbyint(mn / 256.0);            // Python's round(): half to even
    p->ks = ks > 1 ? ks : 1;
    p->h2 = H / p->ks; p->w2 = W / p->ks;
    build_vif_kernels(p->vifk);
    memset(&p->fc, 0, sizeof(p->fc));
    memset(&p->nc, 0, sizeof(p->nc));
    if (p->fft_ok) {
        p->nmax = H > W ? H : W;
        p->tw.resize((size_t)p->nmax);
        for (int k = 0; k < p->nmax / 2; ++k) {
            const double a = -2.0 * kPi * (double)k / (double)p->nmax;
            p->tw[2 * k] = cos(a);
            p->tw[2 * k + 1] = sin(a);
        }
        build_nqm_bands(p);
        build_fsim_bank(p);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {         // without a device the plan serves ipdm_metrics_table only
        // a failed upload frees what was uploaded and the plan itself before it reports
#define UP(dst, vec)                                                                                                        \
    if (!p->vec.empty()) {                                                                                                  \
        hipError_t e_ = hipMalloc((void **)&p->dst, p->vec.size() * sizeof(double));                                        \
        if (e_ == hipSuccess) e_ = hipMemcpy(p->dst, p->vec.data(), p->vec.size() * sizeof(double), hipMemcpyHostToDevice); \
        if (e_ != hipSuccess) {                                                                                             \
            set_error("metrics_plan_create: upload of " #vec " failed: %s", hipGetErrorString(e_));                        \
            ipdm_metrics_plan_destroy(p);                                                                                   \
            return IPDM_ERR_HIP;                                                                                            \
        }                                                                                                                   \
    }
        UP(d_vifk, vifk)
        UP(d_tw, tw)
        UP(d_bands, bands)
        UP(d_filt, filt)
#undef UP
    } else {
        (void)hipGetLastError();
    }
    *out = p;
    return IPDM_OK;
}

extern "C" int ipdm_metrics_plan_destroy(ipdm_metrics_plan *p)
{
    if (!p) return IPDM_OK;
    if (p->d_vifk) (void)hipFree(p->d_vifk);
    if (p->d_tw) (void)hipFree(p->d_tw);
    if (p->d_bands) (void)hipFree(p->d_bands);
    if (p->d_filt) (void)hipFree(p->d_filt);
    delete p;
    return IPDM_OK;
}

extern "C" size_t ipdm_metrics_workspace_bytes(const ipdm_metrics_plan *p, int32_t B, uint32_t mask)
{
    if (!p || B <= 0) return 0;
    if (!p->fft_ok) mask &= ~(uint32_t)(M_NQM | M_FSIM);
    return carve(p, B, mask, nullptr, nullptr);
}

extern "C" int64_t ipdm_metrics_table(const ipdm_metrics_plan *p, int32_t which, void *host_out, int64_t cap)
{
    if (!p) { set_error("metrics_table: null plan"); return IPDM_ERR_INVALID; }
    const double *src = nullptr;
    int64_t n = 0;
    if (which >= 0 && which < 25 && !p->fft_ok) {
        set_error("metrics_table: a %d x %d plan has no frequency-domain tables", p->H, p->W);
        return IPDM_ERR_UNSUPPORTED;
    }
    if (which >= 0 && which < 6) { n = (int64_t)p->H * p->W; src = p->bands.data() + (size_t)which * n; }
    else if (which >= 6 && which < 22) { n = (int64_t)p->h2 * p->w2; src = p->filt.data() + (size_t)(which - 6) * n; }
    else if (which == 22) { n = 4; src = p->fc.sum_an2; }
    else if (which == 23) { n = 4; src = p->fc.sum_aiaj; }
    else if (which == 24) { n = 4; src = p->fc.sum_f0sq; }
    else if (which == 25) { n = (int64_t)p->vifk.size(); src = p->vifk.data(); }
    else { set_error("metrics_table: bad selector %d", which); return IPDM_ERR_INVALID; }
    if (host_out) {
        if (cap < n) { set_error("metrics_table: capacity %ld < %ld", (long)cap, (long)n); return IPDM_ERR_INVALID; }
        memcpy(host_out, src, (size_t)n * sizeof(double));
    }
    return n;
}

extern "C" int ipdm_metrics(ipdm_metrics_plan *p, const float *d_ref, int64_t ref_stride, const float *d_img, int32_t B, uint32_t mask,
                            double *d_out, void *d_ws, size_t ws_bytes, void *stream)
{
    IPDM_REQUIRE(p && d_ref && d_img && d_out && d_ws && B > 0, "metrics: bad argument");
    IPDM_REQUIRE(mask != 0 && (mask & ~31u) == 0, "metrics: mask 0x%x names no metric or an unknown one", mask);
    const int H = p->H, W = p->W;
    const long n = (long)H * W;
    IPDM_REQUIRE(ref_stride == 0 || ref_stride == n, "metrics: ref_stride must be 0 or H*W");
    if ((mask & (M_NQM | M_FSIM)) && !p->fft_ok) {
        set_error("metrics: nqm / fsim need H and W to be powers of two in 64 .. 1024 (plan is %d x %d); score them on the host", H, W);
        return IPDM_ERR_UNSUPPORTED;
    }
    IPDM_REQUIRE(p->d_vifk, "metrics: the plan was created without a device");
    Ws w;
    const size_t need = carve(p, B, mask, d_ws, &w);
    if (ws_bytes < need) { set_error("metrics: workspace %zu < %zu bytes", ws_bytes, need); return IPDM_ERR_WORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(256);
    const dim3 gn(cdiv(n, 256), B);

    hipLaunchKernelGGL(prep_kernel, gn, blk, 0, st, d_ref, (long)ref_stride, d_img, w.R, w.I, n);
    if (mask & M_PSNR) {
        hipLaunchKernelGGL(sqerr_kernel, gn, blk, 0, st, w.R, w.I, w.T0, n);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T0, n, n, 0L, w.acc, (int)A_SSE);
    }
    const long n_ssim = (long)(H - 10) * (W - 10);
    if (mask & M_SSIM) {
        hipLaunchKernelGGL(ssim_kernel, dim3(cdiv(n_ssim, 256), B), blk, 0, st, w.R, w.I, w.T0, H, W, n);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T0, n_ssim, n, 0L, w.acc, (int)A_SSIM);
    }
    if (mask & M_VIF) {
        int hs[4], wsz[4];
        vif_dims(H, W, hs, wsz);
        const long ps = n / 4 + 1;
        const double *cx = w.R, *cy = w.I;
        long cstride = n;
        double mult = 255.0;
        for (int s = 0; s < 4; ++s) {
            const int kn = (1 << (4 - s)) + 1;
            const double *k = p->d_vifk + vif_kernel_offset(s);
            if (s > 0) {
                double *dx = w.P[(s & 1) ? 0 : 2], *dy = w.P[(s & 1) ? 1 : 3];
                hipLaunchKernelGGL(vif_down_kernel, dim3(cdiv((long)hs[s] * wsz[s], 256), B), blk, 0, st, cx, cy, hs[s - 1], wsz[s - 1], cstride,
                                   mult, k, kn, dx, dy, ps);
                cx = dx; cy = dy; cstride = ps; mult = 1.0;
            }
            const long no = (long)(hs[s] - kn + 1) * (wsz[s] - kn + 1);
            hipLaunchKernelGGL(vif_stats_kernel, dim3(cdiv(no, 256), B), blk, 0, st, cx, cy, hs[s], wsz[s], cstride, mult, k, kn, w.T0, w.T1, n);
            hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T0, no, n, 0L, w.acc, (int)A_VNUM + s);
            hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T1, no, n, 0L, w.acc, (int)A_VDEN + s);
        }
    }
    if (mask & M_NQM) {
        hipLaunchKernelGGL(pack_kernel, gn, blk, 0, st, w.R, w.I, w.Z, n);
        fft2d(w.Z, B, H, W, p, 0, st);
        hipLaunchKernelGGL(nqm_mult_kernel, dim3(cdiv(n, 256), B, 6), blk, 0, st, w.Z, p->d_bands, w.C, n);
        fft2d(w.C, B * 6, H, W, p, 1, st);
        hipLaunchKernelGGL(nqm_point_kernel, gn, blk, 0, st, w.C, p->nc, w.T0, w.T1, n);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T0, n, n, 0L, w.acc, (int)A_NQ1);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T1, n, n, 0L, w.acc, (int)A_NQ2);
    }
    if (mask & M_FSIM) {
        const int h2 = p->h2, w2 = p->w2;
        const long n2 = (long)h2 * w2;
        const dim3 g2(cdiv(n2, 256), B);
        hipLaunchKernelGGL(fsim_down_kernel, g2, blk, 0, st, w.R, w.I, H, W, p->ks, h2, w2, w.FA, w.FB, w.Z);
        fft2d(w.Z, B, h2, w2, p, 0, st);
        for (int o = 0; o < 4; ++o) {
            hipLaunchKernelGGL(fsim_mult_kernel, dim3(cdiv(n2, 256), B, 4), blk, 0, st, w.Z, p->d_filt + (size_t)o * 4 * n2, h2, w2, w.C);
            fft2d(w.C, B * 8, h2, w2, p, 1, st);
            hipLaunchKernelGGL(fsim_pc_kernel, dim3(cdiv(n2, 256), B, 2), blk, 0, st, w.C, n2, w.An, w.En, w.E0);
            hipLaunchKernelGGL(select_kernel, dim3(2, 2 * B), dim3(1024), 0, st, w.E0, n2, w.med);
            hipLaunchKernelGGL(fsim_acc_kernel, dim3(cdiv(n2, 256), 2 * B), blk, 0, st, w.An, w.En, w.med, p->fc, o, n2, w.Eall, w.Aall);
        }
        hipLaunchKernelGGL(fsim_final_kernel, g2, blk, 0, st, w.FA, w.FB, w.Eall, w.Aall, h2, w2, w.T0, w.T1, n);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T0, n2, n, 0L, w.acc, (int)A_FS1);
        hipLaunchKernelGGL(reduce_kernel, dim3(1, B), dim3(1024), 0, st, w.T1, n2, n, 0L, w.acc, (int)A_FS2);
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(1), 0, st, w.acc, d_out, mask, (double)n, (double)n_ssim);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}
