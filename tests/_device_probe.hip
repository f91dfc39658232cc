// _device_probe.hip -- test-only entry points onto the device functions of mbb_math.hip.h,
// mbb_device.hip.h, mbb_stretch.hip.h and mbb_gammq.hip.h (tests/test_device_math_gpu.py, tests/test_device_math_cpu.py,
// tests/test_sampler_statistics_gpu.py, tests/test_goodness_gpu.py).  Never part of the
// product library: tests/_device_probe.py compiles it, together with csrc/mbb_host_tables.cpp (the
// builder of the polynomial tables the product uploads), into tests/device_probe/libmbb_device_probe.so with the
// product's own device flags.
//
// With MBB_MATH_HOST (g++, no HIP) only probe_math and probe_poly exist and run the host variant of
// mbb_math.hip.h on the CPU: the same entry points, so the CPU suite drives the same ulp machinery.
//
// Every entry point takes HOST pointers, checks its arguments, copies, launches, synchronises and
// returns 0 or a negative code: -1 bad arguments, -2 an input outside the probed function's domain
// (nothing is launched), -3 a HIP error.  Kernels index nothing by a value they were handed except
// polyrow_eval's row, and that is checked on the host before the launch.
#include <math.h>
#include <stdint.h>
#include <vector>

#include "../mbb_emcee_amd/csrc/mbb_host_tables.h"

enum { PROBE_OK = 0, PROBE_ERR_ARG = -1, PROBE_ERR_DOMAIN = -2, PROBE_ERR_HIP = -3 };
enum { OP_EXP = 0, OP_EXPM1 = 1, OP_LOG = 2, OP_DIV = 3, OP_EXP_T = 4, OP_GAMMQ = 5, OP_COUNT = 6 };

// OP_GAMMQ: x = chisq (anything), y = nb as a double, which must be an integer in [1, 256] (NaN fails the comparisons)
static int gammq_domain_ok(const double *y, long n)
{
    for (long i = 0; i < n; ++i)
        if (!(y[i] >= 1.0 && y[i] <= 256.0 && y[i] == (double)(int)y[i])) return 0;
    return 1;
}

// X = 8 x must name a row of the table: [0, 8 * 48] for b, [0, 8 * 37] for C (NaN fails both comparisons)
static int poly_domain_ok(int which, const double *X, long n)
{
    const double top = which == 0 ? 8.0 * 48 : 8.0 * 37;
    for (long i = 0; i < n; ++i)
        if (!(X[i] >= 0.0 && X[i] <= top)) return 0;
    return 1;
}

#ifdef MBB_MATH_HOST
// ------------------------------------------------------------------ host build
#include "../mbb_emcee_amd/csrc/mbb_math.hip.h"
#include "../mbb_emcee_amd/csrc/mbb_gammq.hip.h"

extern "C" int probe_is_host(void) { return 1; }

extern "C" int probe_math(int op, const double *x, const double *y, long n, double *out)
{
    if (op < 0 || op >= OP_COUNT || !x || !out || n <= 0 || ((op == OP_DIV || op == OP_GAMMQ) && !y)) return PROBE_ERR_ARG;
    if (op == OP_GAMMQ && !gammq_domain_ok(y, n)) return PROBE_ERR_DOMAIN;
    for (long i = 0; i < n; ++i) {
        switch (op) {
        case OP_EXP: out[i] = mbbm::m_exp(x[i]); break;
        case OP_EXPM1: out[i] = mbbm::m_expm1(x[i]); break;
        case OP_LOG: out[i] = mbbm::m_log(x[i]); break;
        case OP_DIV: out[i] = mbbm::m_div(x[i], y[i]); break;
        case OP_GAMMQ: out[i] = mbbm::m_gammq_half((int)y[i], x[i]); break;
        default: out[i] = mbbm::m_exp_t(x[i], mbbm::kExp2Tab); break;
        }
    }
    return PROBE_OK;
}

extern "C" int probe_poly(int which, const double *X, long n, double *out)
{
    if ((which != 0 && which != 1) || !X || !out || n <= 0) return PROBE_ERR_ARG;
    if (!poly_domain_ok(which, X, n)) return PROBE_ERR_DOMAIN;
    std::vector<double> b, c;
    mbbh::build_poly_tables(b, c);
    const std::vector<double> &tab = which == 0 ? b : c;
    for (long i = 0; i < n; ++i) out[i] = mbbm::polyrow_eval(tab.data(), X[i]);
    return PROBE_OK;
}

#else
// ---------------------------------------------------------------- device build
#include <utility>

#include "../mbb_emcee_amd/csrc/mbb_device.hip.h"
#include "../mbb_emcee_amd/csrc/mbb_stretch.hip.h"
#include "../mbb_emcee_amd/csrc/mbb_gammq.hip.h"

using namespace mbbd;

static_assert(mbbm::kPolyStride == mbbh::kPolyStride, "one row stride");
constexpr int kProbeBDoubles = mbbh::kPolyBCount * mbbh::kPolyStride;
constexpr int kProbeCDoubles = mbbh::kPolyCCount * mbbh::kPolyStride;

#define PCHK(expr) do { if ((expr) != hipSuccess) return PROBE_ERR_HIP; } while (0)

namespace {

// a device buffer that frees itself on every return path
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 8); }
    template <typename T> T *as() { return static_cast<T *>(p); }
};

int finite_all(const double *v, long n)
{
    for (long i = 0; i < n; ++i)
        if (!(fabs(v[i]) <= 1.7976931348623157e308)) return 0;
    return 1;
}

int positive_all(const double *v, long n, long stride, long offset)
{
    for (long i = 0; i < n; ++i)
        if (!(v[i * stride + offset] > 0.0)) return 0;
    return 1;
}

int done()
{
    PCHK(hipGetLastError());
    PCHK(hipDeviceSynchronize());
    return PROBE_OK;
}

// ---- primitives: one element per lane
__global__ void k_math(int op, const double *x, const double *y, long n, double *out)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    switch (op) {
    case OP_EXP: r = m_exp(x[i]); break;
    case OP_EXPM1: r = m_expm1(x[i]); break;
    case OP_LOG: r = m_log(x[i]); break;
    case OP_DIV: r = m_div(x[i], y[i]); break;
    case OP_GAMMQ: r = mbbm::m_gammq_half((int)y[i], x[i]); break;
    default: r = m_exp_t(x[i], kExp2Tab); break;
    }
    out[i] = r;
}

// ---- the table look-up (rows validated by the caller)
__global__ void k_poly(const double *tab, const double *X, long n, double *out)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = polyrow_eval(tab, X[i]);
}

// ---- row forms beside lane forms
template <bool ROW, unsigned M1, int K, size_t... I>
__device__ __forceinline__ void vexp_arr(double (&o)[K], const double (&a)[K], std::index_sequence<I...>)
{
    vexp<ROW, M1>(o, a[I]...);
}
template <bool ROW, int K, size_t... I>
__device__ __forceinline__ void vlog_arr(double (&o)[K], const double (&a)[K], std::index_sequence<I...>)
{
    vlog<ROW>(o, a[I]...);
}

// ROW: sixteen lanes per element, every lane of every wave active through the call (the grid is whole
// blocks of a multiple of 64 threads; lanes past the end repeat the last element and store nothing);
// each lane stores what it holds: out[(w * 16 + lane) * K + i].  Lane form: out[w * K + i].
template <bool ROW, bool ISLOG, unsigned M1, int K>
__global__ void k_rows(const double *args, long n, double *out)
{
    const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long w = ROW ? (gid >> 4) : gid;
    const long wc = w < n ? w : n - 1;
    double a[K], o[K];
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = args[wc * K + i];
    if constexpr (ISLOG) vlog_arr<ROW, K>(o, a, std::make_index_sequence<K>());
    else vexp_arr<ROW, M1, K>(o, a, std::make_index_sequence<K>());
    if (w < n) {
        double *dst = ROW ? out + (w * 16 + (threadIdx.x & 15)) * K : out + w * K;
#pragma unroll
        for (int i = 0; i < K; ++i) dst[i] = o[i];
    }
}

// ---- the constructor: vlog of T and lambda0, sed_prologue, sed_peak_wave
constexpr int kProWords = 10;   // normfac xmerge kappa hcokt hokt9 lhokt9 lx0 peak x0 wavemerge
template <bool OPTHIN, bool NOALPHA, bool ROW>
__global__ void k_pro(const double *pars, long n, double nunorm, double lnunorm, double *out,
                      int32_t *status, int32_t *iters)
{
    const long gid = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long w = ROW ? (gid >> 4) : gid;
    const long wc = w < n ? w : n - 1;
    const double T = pars[wc * 5 + 0], beta = pars[wc * 5 + 1], lambda0 = pars[wc * 5 + 2],
                 alpha = pars[wc * 5 + 3], fnorm = pars[wc * 5 + 4];
    double lT, lL = 0.0;
    if constexpr (OPTHIN) {
        double lo[1];
        vlog<ROW>(lo, T);
        lT = lo[0];
    } else {
        double lo[2];
        vlog<ROW>(lo, T, lambda0);
        lT = lo[0]; lL = lo[1];
    }
    const double nan = __builtin_nan("");
    SedScalars s;
    s.normfac = s.xmerge = s.kappa = s.hcokt = s.hokt9 = s.lhokt9 = nan;
    s.lx0 = 0.0;
    int it = 0;
    int st = sed_prologue<OPTHIN, NOALPHA, ROW>(T, beta, alpha, fnorm, lT, lL, nunorm, lnunorm, s, &it);
    double peak = nan;
    if (st == ROW_OK) {
        int pst;
        peak = sed_peak_wave<OPTHIN, ROW>(T, beta, OPTHIN ? 0.0 : s.lx0, s.hcokt, pst);
        if (pst != ROW_OK) st = pst;
    }
    // (the row form stores from a different lane of the row for each element)
    if (w < n && (!ROW || (int)(threadIdx.x & 15) == (int)(w & 15))) {
        double *o = out + w * kProWords;
        o[0] = s.normfac; o[1] = s.xmerge; o[2] = s.kappa; o[3] = s.hcokt; o[4] = s.hokt9;
        o[5] = s.lhokt9; o[6] = s.lx0; o[7] = peak;
        o[8] = OPTHIN ? nan : s.hcokt / lambda0;
        o[9] = NOALPHA ? nan : s.hcokt / s.xmerge;
        status[w] = st;
        iters[w] = it;
    }
}

// ---- one sample: both forms of fnu_sample, as f_nu in mJy.  The tables sit in LDS as in the fused
// kernels; log(nu) of the table form comes from the host's libm as in build_band_layout.
template <bool OPTHIN, bool NOALPHA>
__global__ void __launch_bounds__(256) k_fnu(const double *pars, const double *freq, const double *lnfreq,
                                             long n, long m, double nunorm, double lnunorm,
                                             const double *pb, const double *pc, double *out_tab,
                                             double *out_plain, int32_t *status)
{
    __shared__ __align__(16) double s_tab[kExp2N];
    __shared__ __align__(16) double s_pb[kProbeBDoubles];
    __shared__ __align__(16) double s_pc[kProbeCDoubles];
    for (int i = threadIdx.x; i < kExp2N; i += blockDim.x) s_tab[i] = kExp2Tab[i];
    for (int i = threadIdx.x; i < kProbeBDoubles; i += blockDim.x) s_pb[i] = pb[i];
    for (int i = threadIdx.x; i < kProbeCDoubles; i += blockDim.x) s_pc[i] = pc[i];
    __syncthreads();
    const SampleTabs tabs = {s_tab, s_pb, s_pc};
    const long idx = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (idx >= n * m) return;
    const long r = idx / m;
    const double T = pars[r * 5 + 0], beta = pars[r * 5 + 1], lambda0 = pars[r * 5 + 2],
                 alpha = pars[r * 5 + 3], fnorm = pars[r * 5 + 4];
    SedScalars s;
    s.normfac = s.xmerge = s.kappa = s.hcokt = s.hokt9 = s.lhokt9 = __builtin_nan("");
    s.lx0 = 0.0;
    const int st = sed_prologue<OPTHIN, NOALPHA, false>(T, beta, alpha, fnorm, m_log(T),
                                                        OPTHIN ? 0.0 : m_log(lambda0), nunorm, lnunorm, s);
    double vt = __builtin_nan(""), vp = vt;
    if (st == ROW_OK) {
        WalkerK k;
        k.peak = 0.0; k.status = st; k.pad = 0;
        make_walker_k<OPTHIN, NOALPHA>(beta, alpha, s, k);
        const double nu = freq[idx];
        vt = k.cq * ((nu * nu) * fnu_sample<OPTHIN, NOALPHA, true, false>(k, nu, lnfreq[idx], &tabs));
        vp = fnu_sample<OPTHIN, NOALPHA, false, true>(k, nu, m_log(nu));
    }
    out_tab[idx] = vt;
    out_plain[idx] = vp;
    if (idx % m == 0) status[r] = st;
}

template <typename F>
int dispatch4(int opthin, int noalpha, F f)
{
    if (opthin) return noalpha ? f(std::true_type(), std::true_type()) : f(std::true_type(), std::false_type());
    return noalpha ? f(std::false_type(), std::true_type()) : f(std::false_type(), std::false_type());
}

int check_pars(const double *pars, long n, int opthin)
{
    if (!finite_all(pars, n * 5)) return 0;
    if (!positive_all(pars, n, 5, 0)) return 0;                      // T
    if (!opthin && !positive_all(pars, n, 5, 2)) return 0;           // lambda0 (its log is taken)
    return 1;
}

}  // namespace

extern "C" int probe_is_host(void) { return 0; }

extern "C" int probe_math(int op, const double *x, const double *y, long n, double *out)
{
    if (op < 0 || op >= OP_COUNT || !x || !out || n <= 0 || ((op == OP_DIV || op == OP_GAMMQ) && !y)) return PROBE_ERR_ARG;
    if (op == OP_GAMMQ && !gammq_domain_ok(y, n)) return PROBE_ERR_DOMAIN;
    DevBuf dx, dy, dout;
    const size_t bytes = (size_t)n * sizeof(double);
    PCHK(dx.alloc(bytes)); PCHK(dy.alloc(bytes)); PCHK(dout.alloc(bytes));
    PCHK(hipMemcpy(dx.p, x, bytes, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dy.p, op == OP_DIV || op == OP_GAMMQ ? y : x, bytes, hipMemcpyHostToDevice));
    const int threads = 256;
    hipLaunchKernelGGL(k_math, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, 0, op,
                       dx.as<double>(), dy.as<double>(), n, dout.as<double>());
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return PROBE_OK;
}

extern "C" int probe_poly(int which, const double *X, long n, double *out)
{
    if ((which != 0 && which != 1) || !X || !out || n <= 0) return PROBE_ERR_ARG;
    if (!poly_domain_ok(which, X, n)) return PROBE_ERR_DOMAIN;
    std::vector<double> b, c;
    mbbh::build_poly_tables(b, c);
    const std::vector<double> &tab = which == 0 ? b : c;
    DevBuf dt, dx, dout;
    const size_t bytes = (size_t)n * sizeof(double);
    PCHK(dt.alloc(tab.size() * sizeof(double))); PCHK(dx.alloc(bytes)); PCHK(dout.alloc(bytes));
    PCHK(hipMemcpy(dt.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dx.p, X, bytes, hipMemcpyHostToDevice));
    const int threads = 256;
    hipLaunchKernelGGL(k_poly, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, 0,
                       dt.as<double>(), dx.as<double>(), n, dout.as<double>());
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    return PROBE_OK;
}

// The instantiations of vexp / vlog in the product's sources, as (islog, M1, K).  tests/test_device_math_cpu.py
// holds this list to what the sources call.
struct RowInst { int islog; unsigned m1; int k; };
static const RowInst kRowInst[] = {
    {0, 0x08u, 6}, {0, 0x1Eu, 5}, {0, 0x00u, 2}, {0, 0x02u, 2}, {0, 0x01u, 2}, {0, 0x09u, 5}, {0, 0x01u, 1},
    {0, 0x06u, 3}, {1, 0u, 1}, {1, 0u, 2}, {1, 0u, 4}};
constexpr int kRowInstCount = (int)(sizeof(kRowInst) / sizeof(kRowInst[0]));

extern "C" int probe_rows_count(void) { return kRowInstCount; }

extern "C" int probe_rows_describe(int inst, int *islog, unsigned *m1, int *k)
{
    if (inst < 0 || inst >= kRowInstCount || !islog || !m1 || !k) return PROBE_ERR_ARG;
    *islog = kRowInst[inst].islog; *m1 = kRowInst[inst].m1; *k = kRowInst[inst].k;
    return PROBE_OK;
}

template <bool ISLOG, unsigned M1, int K>
static void launch_rows(const double *args, long n, int block, double *out_row, double *out_lane)
{
    const long row_threads = n * 16;
    hipLaunchKernelGGL((k_rows<true, ISLOG, M1, K>), dim3((unsigned)((row_threads + block - 1) / block)), dim3(block),
                       0, 0, args, n, out_row);
    hipLaunchKernelGGL((k_rows<false, ISLOG, M1, K>), dim3((unsigned)((n + block - 1) / block)), dim3(block), 0, 0,
                       args, n, out_lane);
}

// args[n][K]; out_row[n][16][K] (what each lane of the element's row holds); out_lane[n][K].
// exp arguments must be finite, log arguments positive normal doubles.
extern "C" int probe_rows(int inst, const double *args, long n, int block, double *out_row, double *out_lane)
{
    if (inst < 0 || inst >= kRowInstCount || !args || !out_row || !out_lane || n <= 0 || n > (1L << 24) ||
        (block != 64 && block != 256))
        return PROBE_ERR_ARG;
    const RowInst I = kRowInst[inst];
    const long na = n * I.k;
    if (!finite_all(args, na)) return PROBE_ERR_DOMAIN;
    if (I.islog)
        for (long i = 0; i < na; ++i)
            if (!(args[i] >= 2.2250738585072014e-308)) return PROBE_ERR_DOMAIN;
    DevBuf da, dr, dl;
    PCHK(da.alloc((size_t)na * sizeof(double)));
    PCHK(dr.alloc((size_t)na * 16 * sizeof(double)));
    PCHK(dl.alloc((size_t)na * sizeof(double)));
    PCHK(hipMemcpy(da.p, args, (size_t)na * sizeof(double), hipMemcpyHostToDevice));
    const double *a = da.as<double>();
    double *r = dr.as<double>(), *l = dl.as<double>();
    switch (inst) {
    case 0: launch_rows<false, 0x08u, 6>(a, n, block, r, l); break;
    case 1: launch_rows<false, 0x1Eu, 5>(a, n, block, r, l); break;
    case 2: launch_rows<false, 0x00u, 2>(a, n, block, r, l); break;
    case 3: launch_rows<false, 0x02u, 2>(a, n, block, r, l); break;
    case 4: launch_rows<false, 0x01u, 2>(a, n, block, r, l); break;
    case 5: launch_rows<false, 0x09u, 5>(a, n, block, r, l); break;
    case 6: launch_rows<false, 0x01u, 1>(a, n, block, r, l); break;
    case 7: launch_rows<false, 0x06u, 3>(a, n, block, r, l); break;
    case 8: launch_rows<true, 0u, 1>(a, n, block, r, l); break;
    case 9: launch_rows<true, 0u, 2>(a, n, block, r, l); break;
    default: launch_rows<true, 0u, 4>(a, n, block, r, l); break;
    }
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out_row, dr.p, (size_t)na * 16 * sizeof(double), hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(out_lane, dl.p, (size_t)na * sizeof(double), hipMemcpyDeviceToHost));
    return PROBE_OK;
}

extern "C" int probe_prologue_words(void) { return kProWords; }

// pars[n][5] finite, T > 0 (and lambda0 > 0 for the thick model); out[n][probe_prologue_words()]
extern "C" int probe_prologue(int opthin, int noalpha, int row, const double *pars, long n, double wavenorm,
                              int block, double *out, int32_t *status, int32_t *iters)
{
    if (!pars || !out || !status || !iters || n <= 0 || n > (1L << 24) || (block != 64 && block != 256) ||
        !(wavenorm > 0.0) || !finite_all(&wavenorm, 1))
        return PROBE_ERR_ARG;
    if (!check_pars(pars, n, opthin)) return PROBE_ERR_DOMAIN;
    const double nunorm = kUmToGHz / wavenorm, lnunorm = log(nunorm);
    DevBuf dp, dout, dst, dit;
    PCHK(dp.alloc((size_t)n * 5 * sizeof(double)));
    PCHK(dout.alloc((size_t)n * kProWords * sizeof(double)));
    PCHK(dst.alloc((size_t)n * sizeof(int32_t)));
    PCHK(dit.alloc((size_t)n * sizeof(int32_t)));
    PCHK(hipMemcpy(dp.p, pars, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice));
    PCHK(hipMemset(dout.p, 0xff, (size_t)n * kProWords * sizeof(double)));
    PCHK(hipMemset(dst.p, 0xff, (size_t)n * sizeof(int32_t)));
    PCHK(hipMemset(dit.p, 0xff, (size_t)n * sizeof(int32_t)));
    const long threads = row ? n * 16 : n;
    const dim3 grid((unsigned)((threads + block - 1) / block));
    dispatch4(opthin, noalpha, [&](auto OT, auto NA) {
        constexpr bool ot = decltype(OT)::value, na = decltype(NA)::value;
        if (row)
            hipLaunchKernelGGL((k_pro<ot, na, true>), grid, dim3(block), 0, 0, dp.as<double>(), n, nunorm, lnunorm,
                               dout.as<double>(), dst.as<int32_t>(), dit.as<int32_t>());
        else
            hipLaunchKernelGGL((k_pro<ot, na, false>), grid, dim3(block), 0, 0, dp.as<double>(), n, nunorm, lnunorm,
                               dout.as<double>(), dst.as<int32_t>(), dit.as<int32_t>());
        return 0;
    });
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out, dout.p, (size_t)n * kProWords * sizeof(double), hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(status, dst.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(iters, dit.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PROBE_OK;
}

// pars[n][5], freq[n][m] (GHz, positive finite): out_tab and out_plain [n][m] in mJy, status[n]
extern "C" int probe_fnu(int opthin, int noalpha, const double *pars, const double *freq, long n, long m,
                         double wavenorm, double *out_tab, double *out_plain, int32_t *status)
{
    if (!pars || !freq || !out_tab || !out_plain || !status || n <= 0 || m <= 0 || n * m > (1L << 26) ||
        !(wavenorm > 0.0) || !finite_all(&wavenorm, 1))
        return PROBE_ERR_ARG;
    if (!check_pars(pars, n, opthin)) return PROBE_ERR_DOMAIN;
    const long nm = n * m;
    if (!finite_all(freq, nm) || !positive_all(freq, nm, 1, 0)) return PROBE_ERR_DOMAIN;
    const double nunorm = kUmToGHz / wavenorm, lnunorm = log(nunorm);
    std::vector<double> b, c, lnf((size_t)nm);
    mbbh::build_poly_tables(b, c);
    if ((int)b.size() != kProbeBDoubles || (int)c.size() != kProbeCDoubles) return PROBE_ERR_ARG;
    for (long i = 0; i < nm; ++i) lnf[i] = log(freq[i]);
    DevBuf dp, df, dl, db, dc, dt, dq, dst;
    const size_t fb = (size_t)nm * sizeof(double);
    PCHK(dp.alloc((size_t)n * 5 * sizeof(double))); PCHK(df.alloc(fb)); PCHK(dl.alloc(fb));
    PCHK(db.alloc(b.size() * sizeof(double))); PCHK(dc.alloc(c.size() * sizeof(double)));
    PCHK(dt.alloc(fb)); PCHK(dq.alloc(fb)); PCHK(dst.alloc((size_t)n * sizeof(int32_t)));
    PCHK(hipMemcpy(dp.p, pars, (size_t)n * 5 * sizeof(double), hipMemcpyHostToDevice));
    PCHK(hipMemcpy(df.p, freq, fb, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dl.p, lnf.data(), fb, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(db.p, b.data(), b.size() * sizeof(double), hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dc.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
    const int threads = 256;
    const dim3 grid((unsigned)((nm + threads - 1) / threads));
    dispatch4(opthin, noalpha, [&](auto OT, auto NA) {
        hipLaunchKernelGGL((k_fnu<decltype(OT)::value, decltype(NA)::value>), grid, dim3(threads), 0, 0,
                           dp.as<double>(), df.as<double>(), dl.as<double>(), n, m, nunorm, lnunorm,
                           db.as<double>(), dc.as<double>(), dt.as<double>(), dq.as<double>(), dst.as<int32_t>());
        return 0;
    });
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out_tab, dt.p, fb, hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(out_plain, dq.p, fb, hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(status, dst.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PROBE_OK;
}
// ---- the sampler's random draw (csrc/mbb_stretch.hip.h, what the sampler kernels include): one draw per lane
namespace {

__global__ void k_philox(const uint32_t *ctr, const uint32_t *key, long n, uint32_t *out)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    unsigned int c4[4] = {ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]};
    philox4x32(c4, key[2 * i], key[2 * i + 1]);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = c4[k];
}

__global__ void k_stretch_draw(const int32_t *row, const int32_t *half, const unsigned long long *seed, long n,
                               double stretch_a, int c_count, double *zz, int32_t *pj, double *u3)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= n) return;
    double z, u;
    int j;
    stretch_draw(row[i], 0, half[i], seed[i], stretch_a, c_count, z, j, u);
    zz[i] = z; pj[i] = j; u3[i] = u;
}

}  // namespace

// ctr[n][4], key[n][2] -> out[n][4]: Philox4x32-10 of each counter under each key
extern "C" int probe_philox(const uint32_t *ctr, const uint32_t *key, long n, uint32_t *out)
{
    if (!ctr || !key || !out || n <= 0 || n > (1L << 26)) return PROBE_ERR_ARG;
    DevBuf dc, dk, dout;
    const size_t w = sizeof(uint32_t);
    PCHK(dc.alloc((size_t)n * 4 * w)); PCHK(dk.alloc((size_t)n * 2 * w)); PCHK(dout.alloc((size_t)n * 4 * w));
    PCHK(hipMemcpy(dc.p, ctr, (size_t)n * 4 * w, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dk.p, key, (size_t)n * 2 * w, hipMemcpyHostToDevice));
    const int threads = 256;
    hipLaunchKernelGGL(k_philox, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, 0,
                       dc.as<uint32_t>(), dk.as<uint32_t>(), n, dout.as<uint32_t>());
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(out, dout.p, (size_t)n * 4 * w, hipMemcpyDeviceToHost));
    return PROBE_OK;
}

// stretch_draw of state row row[i] (>= 0) in half half[i] (0 or 1) under key seed[i], scale stretch_a > 1, c_count >= 1
// partners to draw from -> zz[n], pj[n], u3[n]
extern "C" int probe_stretch_draw(const int32_t *row, const int32_t *half, const unsigned long long *seed, long n,
                                  double stretch_a, int c_count, double *zz, int32_t *pj, double *u3)
{
    if (!row || !half || !seed || !zz || !pj || !u3 || n <= 0 || n > (1L << 26) || c_count < 1 ||
        !(stretch_a > 1.0) || !finite_all(&stretch_a, 1))
        return PROBE_ERR_ARG;
    for (long i = 0; i < n; ++i)
        if (row[i] < 0 || (half[i] != 0 && half[i] != 1)) return PROBE_ERR_DOMAIN;
    DevBuf dr, dh, ds, dz, dj, du;
    PCHK(dr.alloc((size_t)n * 4)); PCHK(dh.alloc((size_t)n * 4)); PCHK(ds.alloc((size_t)n * 8));
    PCHK(dz.alloc((size_t)n * 8)); PCHK(dj.alloc((size_t)n * 4)); PCHK(du.alloc((size_t)n * 8));
    PCHK(hipMemcpy(dr.p, row, (size_t)n * 4, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(dh.p, half, (size_t)n * 4, hipMemcpyHostToDevice));
    PCHK(hipMemcpy(ds.p, seed, (size_t)n * 8, hipMemcpyHostToDevice));
    const int threads = 256;
    hipLaunchKernelGGL(k_stretch_draw, dim3((unsigned)((n + threads - 1) / threads)), dim3(threads), 0, 0,
                       dr.as<int32_t>(), dh.as<int32_t>(), ds.as<unsigned long long>(), n, stretch_a, c_count,
                       dz.as<double>(), dj.as<int32_t>(), du.as<double>());
    const int rc = done();
    if (rc) return rc;
    PCHK(hipMemcpy(zz, dz.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(pj, dj.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    PCHK(hipMemcpy(u3, du.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return PROBE_OK;
}
#endif
