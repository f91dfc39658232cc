// mbb_hip.hip -- host side and C-ABI of the MI355X likelihood hot path (gfx950).
//
// The kernels are in mbb_kernels.hip.h (one fused kernel per model variant
// evaluates, for a batch of walkers, prologue -> f_nu on every passband sample ->
// band fluxes -> chi-square / covariance form -> limits and priors -> lnL, i.e. n
// calls of the reference's likelihood.__call__, likelihood.py:790-834, in one
// launch).  This file owns contexts, device buffers, launch geometry, the sampler
// driver and the RCCL plumbing.  See include/mbb_hip.h for the boundary and
// DESIGN.md for the data layout.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <functional>
#include <string>
#include <type_traits>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/mbb_hip.h"
#include "mbb_device.hip.h"
#include "mbb_kernels.hip.h"
#include "mbb_summary.hip.h"
#include "mbb_diag.hip.h"
#include "mbb_marginals.hip.h"
#include "mbb_predict.hip.h"
#include "mbb_goodness.hip.h"
#include "mbb_map.hip.h"
#include "mbb_evidence.hip.h"
#include "mbb_pointwise.hip.h"
#include "mbb_reweight.hip.h"
#include "mbb_population.hip.h"
#include "mbb_draws.hip.h"

// SMODE 6 is instantiated in mbb_flow.hip (its own compiler flags)
#define MBB_FLOW_EXT(OT, NA)                                                    \
    extern template __global__ void k_lnlike<OT, NA, 6, false>(const LikeArgs); \
    extern template __global__ void k_lnlike<OT, NA, 6, true>(const LikeArgs);
MBB_FLOW_EXT(false, false)
MBB_FLOW_EXT(false, true)
MBB_FLOW_EXT(true, false)
MBB_FLOW_EXT(true, true)
#undef MBB_FLOW_EXT
// ... and so is k_flowm, sampler form 7 (mbb_flowm.hip.h; its LDS plan is in mbb_lds_plans.hip.h)
template <bool OPTHIN, bool NOALPHA, bool STAGE, int NP>
__global__ void k_flowm(const LikeArgs a);
#define MBB_FLOWM_EXT(OT, NA)                                                   \
    extern template __global__ void k_flowm<OT, NA, false, 1>(const LikeArgs); \
    extern template __global__ void k_flowm<OT, NA, true, 1>(const LikeArgs);
MBB_FLOWM_EXT(false, false)
MBB_FLOWM_EXT(false, true)
MBB_FLOWM_EXT(true, false)
MBB_FLOWM_EXT(true, true)
#undef MBB_FLOWM_EXT
// ... and k_flowa, form 9: the same resident run with the constructor a half-step ahead (mbb_flowa.hip.h)
template <bool OPTHIN, bool NOALPHA, bool STAGE>
__global__ void k_flowa(const LikeArgs a);
#define MBB_FLOWA_EXT(OT, NA)                                               \
    extern template __global__ void k_flowa<OT, NA, false>(const LikeArgs); \
    extern template __global__ void k_flowa<OT, NA, true>(const LikeArgs);
MBB_FLOWA_EXT(false, false)
MBB_FLOWA_EXT(false, true)
MBB_FLOWA_EXT(true, false)
MBB_FLOWA_EXT(true, true)
#undef MBB_FLOWA_EXT
// ... and k_serve, the likelihood of given rows as a kernel that stays resident between boundary calls (mbb_serve.hip.h)
template <bool OPTHIN, bool NOALPHA, bool STAGE, bool OVL>
__global__ void k_serve(const LikeArgs a);
#define MBB_SERVE_EXT(OT, NA)                                                      \
    extern template __global__ void k_serve<OT, NA, false, false>(const LikeArgs); \
    extern template __global__ void k_serve<OT, NA, true, false>(const LikeArgs);  \
    extern template __global__ void k_serve<OT, NA, false, true>(const LikeArgs);  \
    extern template __global__ void k_serve<OT, NA, true, true>(const LikeArgs);
MBB_SERVE_EXT(false, false)
MBB_SERVE_EXT(false, true)
MBB_SERVE_EXT(true, false)
MBB_SERVE_EXT(true, true)
#undef MBB_SERVE_EXT
constexpr int kServePasses = 2;               // rows a workgroup of a resident server takes of one request, at most

// Every variant of the likelihood family that launch_packed starts has ONE slot: its kernel, its module handle and its
// dynamic-LDS grant are filed under it.  Within a kind of kernel the model comes first -- (opthin ? 2 : 0) | (noalpha ? 1 : 0)
// -- then the kind's own choices, `sub`:
//   k_lnlike  2 x (SMODE 0, 1, 2, 6 as 0, 1, 2, 3) + staged      k_flowm, k_flowa  staged
//   k_serve   2 x overlapped + staged
enum KernelKind { kLnlike, kFlowm, kFlowa, kServe, kKinds };
constexpr int kModels = 4;
constexpr int kKindWidth[kKinds] = {8, 2, 2, 4};
constexpr int kind_base(int k) { return k == 0 ? 0 : kind_base(k - 1) + kModels * kKindWidth[k - 1]; }
constexpr int kNumSlots = kind_base(kKinds);
constexpr int kernel_slot(KernelKind k, int model, int sub) { return kind_base(k) + model * kKindWidth[k] + sub; }

#define MBB_MODELS(V) V(false, false), V(false, true), V(true, false), V(true, true)
#define MBB_LNLIKE_V(OT, NA)                                                                            \
    k_lnlike<OT, NA, 0, false>, k_lnlike<OT, NA, 0, true>, k_lnlike<OT, NA, 1, false>, k_lnlike<OT, NA, 1, true>, \
        k_lnlike<OT, NA, 2, false>, k_lnlike<OT, NA, 2, true>, k_lnlike<OT, NA, 6, false>, k_lnlike<OT, NA, 6, true>
#define MBB_FLOWM_V(OT, NA) k_flowm<OT, NA, false, 1>, k_flowm<OT, NA, true, 1>
#define MBB_FLOWA_V(OT, NA) k_flowa<OT, NA, false>, k_flowa<OT, NA, true>
#define MBB_SERVE_V(OT, NA) \
    k_serve<OT, NA, false, false>, k_serve<OT, NA, true, false>, k_serve<OT, NA, false, true>, k_serve<OT, NA, true, true>
static void (*const g_kernel[kNumSlots])(const LikeArgs) = {MBB_MODELS(MBB_LNLIKE_V), MBB_MODELS(MBB_FLOWM_V),
                                                            MBB_MODELS(MBB_FLOWA_V), MBB_MODELS(MBB_SERVE_V)};
#undef MBB_MODELS
#undef MBB_LNLIKE_V
#undef MBB_FLOWM_V
#undef MBB_FLOWA_V
#undef MBB_SERVE_V
#include "mbb_host_tables.h"
#include "mbb_options.h"
#include "mbb_owned.h"
#include "mbb_registry.h"

static_assert(kPolyBDoubles == mbbh::kPolyBCount * mbbh::kPolyStride && mbbh::kPolyStride == mbbm::kPolyStride, "poly table size");
static_assert(kPolyCDoubles == mbbh::kPolyCCount * mbbh::kPolyStride, "poly table size");
static_assert(sizeof(mbbh::Unit) == sizeof(int4) && sizeof(mbbh::SlotRange) == sizeof(int2), "layout");


// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const char *what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (code == MBB_ERR_HIP)
        snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else
        snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

#define HIPCHK(call)                                                   \
    do {                                                               \
        hipError_t e_ = (call);                                        \
        if (e_ != hipSuccess) return fail(MBB_ERR_HIP, #call, e_);     \
    } while (0)

typedef void *ncclComm_t_;
struct UniqueId { char internal[128]; };
struct RcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(ncclComm_t_ *, int, UniqueId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, ncclComm_t_, hipStream_t) = nullptr;
    int (*CommDestroy)(ncclComm_t_) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;

static int load_rccl()
{
    if (g_rccl.handle) return MBB_OK;
    // A copy that is in the process already first (by its soname): a launcher that has imported torch brings torch's
    // own librccl / libamdhip64 / libhsa-runtime64 along, this library then runs on THAT HIP runtime (same soname), and
    // a second RCCL from the system path would bring a second HSA runtime with it.
    // MBB_RCCL_LIB names the library outright: a site's own RCCL build -- and what the one-GPU tests use to run the
    // N > 1 code with ranks that share a device (tests/rccl_standin/).  A path that does not load is an error, never
    // a reason to look elsewhere.
    void *h = nullptr;
    if (const char *named = getenv("MBB_RCCL_LIB")) {
        if (*named && !(h = dlopen(named, RTLD_NOW | RTLD_LOCAL)))
            return fail(MBB_ERR_RCCL, "cannot load the library MBB_RCCL_LIB names");
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(MBB_ERR_RCCL, "cannot load librccl.so");
    g_rccl.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(ncclComm_t_ *, int, UniqueId, int))dlsym(h, "ncclCommInitRank");
    g_rccl.AllGather = (int (*)(const void *, void *, size_t, int, ncclComm_t_, hipStream_t))
        dlsym(h, "ncclAllGather");
    g_rccl.CommDestroy = (int (*)(ncclComm_t_))dlsym(h, "ncclCommDestroy");
    g_rccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(MBB_ERR_RCCL, "librccl.so lacks the expected nccl* symbols");
    g_rccl.handle = h;
    return MBB_OK;
}

// The runtime under the owners of mbb_owned.h: every device and pinned block the library keeps is made and freed here.
using mbbo::DevBuf;
using mbbo::Dev;
using mbbo::Pin;
using mbbo::ResultBlock;
int mbbo::dev_alloc(void **p, size_t bytes, DevKind kind)
{
    if (kind == kDevFine) HIPCHK(hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained));
    else HIPCHK(hipMalloc(p, bytes));
    return MBB_OK;
}
int mbbo::dev_free(void *p)
{
    HIPCHK(hipFree(p));
    return MBB_OK;
}
int mbbo::pin_alloc(void **p, void **alias, size_t bytes, PinKind kind)
{
    // mapped AND coherent (fine-grained): a kernel's stores to the block must become visible to the polling host
    // while the kernel is still running, whatever HIP_HOST_COHERENT defaults to
    HIPCHK(hipHostMalloc(p, bytes, kind == kPinMapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
    if (kind == kPinMapped) {
        const hipError_t e = hipHostGetDevicePointer(alias, *p, 0);
        if (e != hipSuccess) { (void)pin_free(*p); return fail(MBB_ERR_HIP, "hipHostGetDevicePointer(alias, *p, 0)", e); }
    }
    return MBB_OK;
}
int mbbo::pin_free(void *p)
{
    HIPCHK(hipHostFree(p));
    return MBB_OK;
}

// Two events, made when first asked for and destroyed with whatever holds them.
struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    EventPair() = default;
    EventPair(const EventPair &) = delete;
    ~EventPair() { for (hipEvent_t ev : e) if (ev) (void)hipEventDestroy(ev); }
    int create()
    {
        for (hipEvent_t &ev : e) if (!ev) HIPCHK(hipEventCreate(&ev));
        return MBB_OK;
    }
};

struct mbb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int cu_count = 256, xcds = 8;
    // model
    int opthin = 0, noalpha = 0;
    double wavenorm = 500.0;
    // bands
    int nb = 0, nseg = 0, nunit = 0, npart = 0, nchunk = 0, nq = 0;
    long t_prep_ns = 0, t_launch_ns = 0, t_wait_ns = 0;   // phases of the last mbb_lnlike_batch
    std::vector<double> band_freq, band_wt;   // the bands as mbb_set_bands was given them: sample frequencies [GHz], weights,
    std::vector<int32_t> band_off;            // ... and offsets [nb + 1] (the goodness of fit sums them in this order)
    int simd_chunks[4] = {0, 0, 0, 0};   // chunks dealt to each SIMD position by the unit table
    // Every device or pinned block below is an owner (mbb_owned.h), grouped with its capacity: it is remade through grow()
    // and freed with the context.
    struct BandTabs {
        Dev<double> nu, lnnu, wt;
        Dev<int4> unit_tab;
        Dev<int2> band_rng;
        Dev<int32_t> tail_slot;
    } band;
    double *d_poly_b = nullptr, *d_poly_c = nullptr;     // piecewise polynomials of the sample loop: the device's, not the context's
    // data
    int data_nb = 0, has_cov = 0, nsrc = 1;
    struct Data { Dev<double> flux, ivar, invcov; } data;
    // limits and priors (likelihood.py:73, :83-85 defaults)
    double lowlim[5] = {1, 0.1, 1, 0.1, 1e-3};
    double uplim[6] = {INFINITY, 20.0, INFINITY, 20.0, INFINITY, INFINITY};
    uint32_t has_uplim = (1u << 1) | (1u << 3);
    double gmean[6] = {0, 0, 0, 0, 0, 0};
    double givar[6] = {1, 1, 1, 1, 1, 1};
    uint32_t has_gprior = 0;
    // staging for the host-in / host-out path
    struct Boundary {
        size_t cap = 0, cap_flux = 0;             // rows; model fluxes
        Dev<double> d_pars, d_lnl, d_mflux;
        Dev<int32_t> d_status;
        Pin<double> h_pars, h_lnl, h_mflux;       // pinned, and (dv()) as the device addresses them
        Pin<int32_t> h_status;
        Dev<double> w_pars{mbbo::kDevFine};       // device memory the host writes through the PCIe BAR (fine-grained), or empty
    } bnd;
    // the served boundary (k_serve, mbb_serve.hip.h): a kernel that stays resident between a host-driven sampler's calls
    struct ServeMem {
        Dev<unsigned long long> w_door{mbbo::kDevFine};   // its doorbell: a word of fine-grained device memory the host writes through the BAR
        Pin<double> h_srv;                        // pinned: a server's result records [row]{lnl, status as a 64-bit integer}
        Pin<unsigned long long> h_gone;           // pinned: the number of the last request a server saw before it left (0: still there)
    } srv;
    // The serve state below is a context's own -- except that a SIBLING context coming to the device tells this one's
    // server to leave (yield_server), possibly from another thread (ctypes and the _mbbfast extension release the GIL).
    // srv_mu guards it: held by the owner for the whole of mbb_lnlike_call and of use(), taken by a visitor (try_lock
    // under g_dev_mutex, so that a context cannot be destroyed between being found and being locked) around serve_stop.
    // Lock order: ctx.srv_mu, then g_dev_mutex; a thread waits for another context's srv_mu only while its own context
    // is NOT the device's server, and the server's owner never waits for a sibling: no cycle.
    std::mutex srv_mu;
    bool serving = false;
    unsigned long long srv_seq = 0;           // requests so far (the doorbell word is request number << 16 | rows)
    int srv_hot = 0;                          // boundary calls in a row with nothing else in between
    long srv_need = 0;                        // ... of which a server is started (0: opt.serve_after).  Doubled, up to 64, every
                                              // time a sibling context's visit sends this context's server away, back to
                                              // opt.serve_after once a server has answered 256 requests: two likelihoods used
                                              // in turns must not spend their time starting and stopping kernels
    long srv_run = 0;                         // requests the present server has answered
    int srv_strikes = 0;                      // servers that had to be given up in a row; three rest the feature
    long srv_rest = 0, srv_rests = 0;         // boundary calls the feature still rests for; how often it has had to
    long srv_requests = 0, srv_fallbacks = 0;
    int srv_grid = 0;                         // workgroups of the server that is resident
    int srv_want = 0;                         // the most rows a call of this context has had (in eights): a server is started that wide
    long srv_resizes = 0;                     // servers that left because they were the wrong width
    int srv_busy = 0;                         // busy processes beside this one, as the latest boundary call counted them
    long srv_t0_ns = 0;                       // when the present server was started
    uint32_t reg_key = 0;                     // the device's name in the cross-process registry (mbb_registry.h): PCI domain:bus:device
    long srv_lease_yields = 0;                // servers sent away because their lease was up
    long srv_peer_yields = 0;                 // servers not started, or sent away, because another process is on the device
    unsigned long long buf_gen = 1;   // mbb_boundary_generation: bumped whenever the blocks below are freed and made anew
    double *call_in = nullptr;   // mbb_boundary_buffers: where the caller writes its rows (w_pars or h_pars)
    size_t call_cap = 0;         // ... and the capacity that answer was given for
    hipFunction_t mod_fn[kNumSlots] = {};   // the kernels' module handles, by slot (kernel_slot)
    struct Gather {                                    // sharded boundary: every rank's lnprob, device / pinned landing place
        Dev<double> d;
        Pin<double> h{mbbo::kPinDefault};
    } gather;
    int large_bar = -1;
    // scratch for SED-level calls
    struct SedWork {
        size_t cap = 0, out_cap = 0;                   // rows; output values
        Dev<double> pars, out;
        Dev<int32_t> status;
        Dev<WalkerK> wk;
    } sed;
    // Work buffers of the chain analyses.  The derived columns of a
    // chain (summary_fill_derived), for the summary and the marginals alike:
    struct DerWork {
        DevBuf der, src, colstatus;           // the columns, the per-source constants, [nsrc][kCols] row-status bits
        std::vector<mbbs::SrcConst> h_src;    // the per-source constants as uploaded (kept until the next call's)
        bool src_in_flight = false;           // ... and whether that upload may still be reading them
    } der;
    // ... the column statistics and the select behind them (grow_stats, grow_select), shared: the analyses are synchronous, one at a time
    struct StatWork { DevBuf part, state, hist; } stat;
    struct SumWork { DevBuf covpart, outbuf; } sum;                             // ... the chain summary (summary_run)
    struct DiagWork {                                                           // ... the chain diagnostics (diag_run)
        DevBuf mean, seq, outbuf;
        size_t lds_granted = 0;               // dynamic-LDS ceiling already requested for k_diag_acf
    } diag;
    struct MargWork { DevBuf extent, range, part1, part2, outbuf; } marg;       // ... the chain marginals (marg_run)
    struct PredWork { DevBuf samples, status, outbuf; } pred;                   // ... the predicted fluxes (pred_run)
    struct DrawWork { DevBuf rows, aux; } draw;     // ... the posterior draws (draws_run): the compact block, its lnprob and index
    struct GoodWork { DevBuf samples, band, mf, rows, best, status, outbuf; } good;   // ... and the goodness of fit (good_run)
    struct MapWork {                                                            // the posterior's maximum (mbb_map_fit)
        DevBuf start, outbuf;
        size_t lds_granted[8] = {};           // whether this context has asked for the dynamic-LDS ceiling, by instantiation of k_map_lm
    } map;
    struct EvWork { DevBuf mom, ints, slab, l1, l2, postq, neff, outbuf; } ev;  // the evidence of a chain (evidence_run)
    struct PwWork { DevBuf cols, part, state, sel, status, outbuf; } pw;        // the out-of-sample fit of a chain (pw_run)
    struct RwWork {                                                             // a chain reweighted under this context's density (rw_run)
        DevBuf slab, cols, count, state, sel, status, wpart, wstate, whist, covpart, entries, outbuf;
    } rw;
    struct PopBlock {                                                           // the population block of a chain (pop_build) and
        DevBuf x, b, count, hyper, part, lsrc, outbuf;                          // the work of its evaluations (pop_eval)
        long long serial = 0, n = 0, per_split = 0;                             // serial: of the last build, never handed out twice
        int nsrc = 0, d = 0, splits = 0;
        bool live = false;                                                      // a block of that serial is there
    } pop;
    mbbopt::Options opt;                       // what mbb_set_option sets: every field, default and bound in mbb_options.h
    long last_prepass = 0;                     // whether the last likelihood launch was preceded by k_walker_pre (launch_rows)
    Dev<double> pre;                           // ... its records
    long last_watch_seen = -1;          // last mbb_lnlike_batch: 1 results seen by the watch, 0 fell back, -1 no watch
    long last_stage = 0;
    EventPair ev_timed;            // mbb_sampler_advance_timed
    long flow_fallbacks = 0;       // one-launch runs that timed out and were redone as a launch train
    // A give-up is a property of the moment (a co-tenant holding CUs), not of the context: the next run
    // takes the one-launch form again.  Only kFlowStrikes give-ups in a row rest it, for kFlowRest runs.
    long flow_strikes = 0, flow_rest = 0;
    size_t lds_granted[kNumSlots] = {};   // dynamic-LDS ceiling already requested, by slot (kernel_slot)
    long last_wpb = 0, last_threads = 0, last_grid = 0, last_smem = 0, last_smode = 0, last_ahead = 0;
    Dev<unsigned long long> stamps;           // diagnostic build only
    // rccl
    ncclComm_t_ comm = nullptr;
    int nranks = 1, rank = 0;
    // one-hop exchange (mbb_xchg_*): one fine-grained allocation per rank, mapped by all peers:
    // [flags: 16 x u64][arrival counter][state rows: xcap x 6 doubles]
    struct XchgState {
        int n = 0, rank = 0, connected = 0;
        int users = 0;                            // samplers whose state rows live in this buffer
        size_t cap_rows = 0;
        unsigned char *peer[16] = {};             // every rank's allocation as mapped here (own = base)
        unsigned long long flow_run = 0;          // one-launch sharded runs so far (the same on every rank)
        unsigned long long seq = 0;               // launches posted so far
    };
    struct Xchg : XchgState {
        Dev<unsigned char> base{mbbo::kDevFine};  // own allocation
        Dev<XchgArgs> d_args;                     // the kernel's view (device memory)
        Dev<FlowX> d_flowx;                       // the one-launch sharded run's view of every rank's copy (device memory)
        static constexpr size_t kHeader = 256;
        // unmaps the peers' allocations, frees its own and is as new
        void close()
        {
            for (int r = 0; r < n; ++r)
                if (r != rank && peer[r]) (void)hipIpcCloseMemHandle(peer[r]);
            base.release(); d_args.release(); d_flowx.release();
            static_cast<XchgState &>(*this) = XchgState();
        }
        ~Xchg() { close(); }
        double *pos6(int r) const { return reinterpret_cast<double *>(peer[r] + kHeader); }
        // behind the rows: the state of a one-launch run (FlowView, mbb_kernels.hip.h), sized for cap_rows
        double *flow(int r) const { return reinterpret_cast<double *>(peer[r] + kHeader + cap_rows * 6 * sizeof(double)); }
        unsigned long long *flags(int r) const { return reinterpret_cast<unsigned long long *>(peer[r]); }
        unsigned int *count() const { return reinterpret_cast<unsigned int *>(base.d() + 128); }
    } x;
};

// How a block of a context is remade bigger (mbbo::DevBuf::grow, PinBuf::grow): big enough already, or the context's
// stream is brought to rest, the old block released and the new one made.
static int sync_stream(mbb_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}
static int grow(mbb_ctx *c, DevBuf &b, size_t bytes) { return b.grow(bytes, [c] { return sync_stream(c); }); }
static int grow(mbb_ctx *c, mbbo::PinBuf &b, size_t bytes) { return b.grow(bytes, [c] { return sync_stream(c); }); }

static int serve_stop(mbb_ctx *c);

// Every entry point but the boundary call comes through here: a resident server (k_serve) is told to leave first --
// it holds the CUs, and its arguments were fixed at its launch -- and the streak of boundary calls ends.
static int yield_server(mbb_ctx *c);
static int use(mbb_ctx *c)
{
    if (!c) return fail(MBB_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));
    std::lock_guard<std::mutex> own(c->srv_mu);
    c->srv_hot = 0;
    if (c->serving) return serve_stop(c);
    return yield_server(c);
}

extern "C" const char *mbb_last_error(void) { return g_err.c_str(); }

extern "C" int mbb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

struct DeviceStatics {
    bool ready = false;
    int cu_count = 0, xcds = 8;
    double *d_poly_b = nullptr, *d_poly_c = nullptr;
    std::vector<hipStream_t> idle_streams;
    std::atomic<int> live{0};        // contexts of this process on the device
    struct mbb_ctx *server = nullptr;    // the context whose k_serve is resident on the device, if any (g_dev_mutex)
    struct mbb_ctx *last_user = nullptr; // the context that came to the device last: "calls in a row" are a context's own
};
static std::mutex g_dev_mutex;
static DeviceStatics g_dev[64];

// Another context of this process has a server resident on c's device: it holds the CUs, so whatever c is about to put on
// its stream would wait for it -- it is told to leave first (and starts again after its own next few calls in a row).
// Called with c->srv_mu held and c NOT serving.
static int yield_server(mbb_ctx *c)
{
    if (c->device < 0 || c->device >= 64) return MBB_OK;
    for (long tries = 0;; ++tries) {
        mbb_ctx *o;
        {
            std::lock_guard<std::mutex> lk(g_dev_mutex);
            o = g_dev[c->device].server;
            if (g_dev[c->device].last_user != c) {
                // (another context was here in between: this one's boundary calls are not "in a row" any more)
                g_dev[c->device].last_user = c;
                c->srv_hot = 0;
            }
            if (!o || o == c) return MBB_OK;
            // found and locked inside one critical section: mbb_ctx_destroy takes the server's name off the device
            // under g_dev_mutex after its own serve_stop, so `o` is alive here and stays so while its srv_mu is held
            if (!o->srv_mu.try_lock()) o = nullptr;
        }
        if (!o) {
            // its owner is inside a call (at most the serve budget, ~0.4 ms): come back
            if ((tries & 15) == 15) std::this_thread::yield(); else __builtin_ia32_pause();
            continue;
        }
        std::lock_guard<std::mutex> theirs(o->srv_mu, std::adopt_lock);
        if (!o->serving) return MBB_OK;            // (it left by itself, or its owner sent it away, in between)
        o->srv_hot = 0;
        o->srv_need = std::min<long>(64, 2 * (o->srv_need > 0 ? o->srv_need : o->opt.serve_after));
        return serve_stop(o);
    }
}

extern "C" int mbb_ctx_create(int device, mbb_ctx **out)
{
    if (!out) return fail(MBB_ERR_ARG, "out is null");
    *out = nullptr;
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(MBB_ERR_ARG, "no such HIP device");
    HIPCHK(hipSetDevice(device));
    // What is the same for every context of a device is made once per process and shared: the device's CU
    // count and the two polynomial tables of the sample loop (read-only; never freed).  A catalogue loop makes
    // a context per source: this took a new one from 6.2 ms to the stream and a few allocations
    // (tools/probe_first_fit.py).
    if (device >= 64) return fail(MBB_ERR_ARG, "device number out of range");
    {
        std::lock_guard<std::mutex> lock(g_dev_mutex);
        DeviceStatics &d = g_dev[device];
        if (!d.ready) {
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, device));
            d.cu_count = prop.multiProcessorCount;
            int xcc = 0;                  // (MI355X: 8 XCDs of 32 CUs; the share of a device is dealt in whole rows of them)
            if (hipDeviceGetAttribute(&xcc, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) (void)hipGetLastError();
            d.xcds = xcc > 0 && d.cu_count % xcc == 0 ? xcc : 8;
            std::vector<double> pb, pc;
            mbbh::build_poly_tables(pb, pc);
            HIPCHK(hipMalloc((void **)&d.d_poly_b, pb.size() * sizeof(double)));
            HIPCHK(hipMalloc((void **)&d.d_poly_c, pc.size() * sizeof(double)));
            HIPCHK(hipMemcpy(d.d_poly_b, pb.data(), pb.size() * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d.d_poly_c, pc.data(), pc.size() * sizeof(double), hipMemcpyHostToDevice));
            d.ready = true;
        }
    }
    mbb_ctx *c = new mbb_ctx();
    c->device = device;
    c->cu_count = g_dev[device].cu_count;
    c->xcds = g_dev[device].xcds;
    c->d_poly_b = g_dev[device].d_poly_b;
    c->d_poly_c = g_dev[device].d_poly_c;
    // A stream costs ~5 ms to create (a hardware queue): the streams of contexts that have gone are kept, idle,
    // for the contexts to come.
    {
        std::lock_guard<std::mutex> lock(g_dev_mutex);
        std::vector<hipStream_t> &pool = g_dev[device].idle_streams;
        if (!pool.empty()) { c->stream = pool.back(); pool.pop_back(); }
    }
    if (!c->stream) {
        // The runtime deals the streams of one priority class to four hardware queues in turn, and a kernel that lands behind
        // a RESIDENT one on its queue (k_serve between a sampler's calls) does not start until that one leaves -- measured:
        // tools/lat_two_residents.hip, 20 ms (the resident kernel's own limit) instead of 50 us for every fourth stream.
        // Streams of another class never share a queue with it.  So the library's streams are of the class applications use
        // least, the least urgent one: whatever the application (torch, a prior of its own on the GPU) puts on its streams is
        // not held up by a resident server.  (By itself the class costs nothing: M1 and M2 the same at any priority.)
        int least = 0, most = 0;
        hipError_t es = hipDeviceGetStreamPriorityRange(&least, &most);
        if (es == hipSuccess && least != most) es = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, least);
        else es = hipErrorNotSupported;
        if (es != hipSuccess) {
            (void)hipGetLastError();
            c->stream = nullptr;
            es = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        }
        if (es != hipSuccess) { delete c; return fail(MBB_ERR_HIP, "hipStreamCreateWithFlags", es); }
    }
    ++g_dev[device].live;
    {
        // the device's name for other processes: its PCI address (the HIP ordinal is renumbered by HIP_VISIBLE_DEVICES)
        int dom = 0, bus = 0, dv = 0;
        if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, device) != hipSuccess) dom = 0;
        if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, device) != hipSuccess) bus = device;
        if (hipDeviceGetAttribute(&dv, hipDeviceAttributePciDeviceId, device) != hipSuccess) dv = 0;
        (void)hipGetLastError();
        c->reg_key = 0x80000000u | ((uint32_t)(dom & 0x7fff) << 16) | ((uint32_t)(bus & 0xff) << 8) | (uint32_t)(dv & 0xff);
        mbbh::registry_join(c->reg_key);
    }
    *out = c;
    return MBB_OK;
}

extern "C" void mbb_ctx_destroy(mbb_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    {
        // (a sibling's visit -- yield_server on another thread -- is either over or has not found this context yet)
        std::lock_guard<std::mutex> own(c->srv_mu);
        if (c->serving) (void)serve_stop(c);
    }
    if (c->device >= 0 && c->device < 64) {
        --g_dev[c->device].live;
        std::lock_guard<std::mutex> lk(g_dev_mutex);
        if (g_dev[c->device].last_user == c) g_dev[c->device].last_user = nullptr;
        if (g_dev[c->device].server == c) g_dev[c->device].server = nullptr;
    }
    mbbh::registry_leave(c->reg_key);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    const hipStream_t stream = c->stream;
    const int device = c->device;
    delete c;       // the exchange, every buffer and the events: the members free themselves
    if (stream) {
        // idle (synchronised above): kept for the next context of this device, up to a handful
        std::lock_guard<std::mutex> lock(g_dev_mutex);
        if (device >= 0 && device < 64 && g_dev[device].idle_streams.size() < 8)
            g_dev[device].idle_streams.push_back(stream);
        else
            (void)hipStreamDestroy(stream);
    }
}

extern "C" int mbb_set_model(mbb_ctx *c, int opthin, int noalpha, double wavenorm)
{
    if (!c) return fail(MBB_ERR_ARG, "null context");
    if (!(wavenorm > 0.0)) return fail(MBB_ERR_ARG, "wavenorm must be positive");
    c->opthin = opthin ? 1 : 0;
    c->noalpha = noalpha ? 1 : 0;
    c->wavenorm = wavenorm;
    return MBB_OK;
}

// (a table is made anew at its exact size, one element at least; the caller has brought the stream to rest)
template <typename T>
static int upload(Dev<T> &b, const std::vector<T> &h)
{
    if (const int rc = b.remake(sizeof(T) * (h.size() ? h.size() : 1))) return rc;
    if (!h.empty())
        HIPCHK(hipMemcpy(b.d(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return MBB_OK;
}

extern "C" int mbb_set_bands(mbb_ctx *c, const double *freq, const double *weight,
                             const int32_t *offsets, int nb)
{
    int rc = use(c);
    if (rc) return rc;
    mbbh::BandLayout L;
    const char *why = "bad band tables";
    if (mbbh::build_band_layout(freq, weight, offsets, nb, (int)c->opt.seg_chunks, c->opt.pack_tails != 0, L, &why))
        return fail(MBB_ERR_ARG, why);
    std::vector<int4> unit_tab(L.unit_tab.size());
    std::vector<int2> band_rng(L.band_rng.size());
    memcpy(unit_tab.data(), L.unit_tab.data(), unit_tab.size() * sizeof(int4));
    memcpy(band_rng.data(), L.band_rng.data(), band_rng.size() * sizeof(int2));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = upload(c->band.nu, L.nu))) return rc;
    if ((rc = upload(c->band.lnnu, L.lnnu))) return rc;
    if ((rc = upload(c->band.wt, L.wt))) return rc;
    if ((rc = upload(c->band.unit_tab, unit_tab))) return rc;
    if ((rc = upload(c->band.band_rng, band_rng))) return rc;
    if ((rc = upload(c->band.tail_slot, L.tail_slot))) return rc;
    c->nb = nb;
    c->band_off.assign(offsets, offsets + nb + 1);
    c->band_freq.assign(freq, freq + offsets[nb]);
    c->band_wt.assign(weight, weight + offsets[nb]);
    c->nchunk = L.nchunk;
    c->nseg = L.nseg;
    c->nunit = L.nunit;
    c->npart = L.npart;
    for (int g = 0; g < 4; ++g) c->simd_chunks[g] = L.simd_chunks[g];
    c->nq = L.nq;
    return MBB_OK;
}

extern "C" int mbb_set_data(mbb_ctx *c, const double *flux, const double *w, int nb, int is_cov)
{
    int rc = use(c);
    if (rc) return rc;
    if (!flux || !w || nb <= 0) return fail(MBB_ERR_ARG, "bad data");
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<double> f(flux, flux + nb);
    if ((rc = upload(c->data.flux, f))) return rc;
    if (is_cov) {
        std::vector<double> m(w, w + (size_t)nb * nb);
        if ((rc = upload(c->data.invcov, m))) return rc;
        std::vector<double> iv(nb, 0.0);
        if ((rc = upload(c->data.ivar, iv))) return rc;
    } else {
        std::vector<double> iv(w, w + nb);
        if ((rc = upload(c->data.ivar, iv))) return rc;
        c->data.invcov.release();
    }
    c->has_cov = is_cov ? 1 : 0;
    c->data_nb = nb;
    c->nsrc = 1;
    return MBB_OK;
}

extern "C" int mbb_set_data_multi(mbb_ctx *c, const double *flux, const double *ivar, int nb, int nsrc)
{
    int rc = use(c);
    if (rc) return rc;
    if (!flux || !ivar || nb <= 0 || nsrc <= 0) return fail(MBB_ERR_ARG, "bad data");
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<double> f(flux, flux + (size_t)nb * nsrc), iv(ivar, ivar + (size_t)nb * nsrc);
    if ((rc = upload(c->data.flux, f))) return rc;
    if ((rc = upload(c->data.ivar, iv))) return rc;
    c->data.invcov.release();
    c->has_cov = 0;
    c->data_nb = nb;
    c->nsrc = nsrc;
    return MBB_OK;
}

extern "C" int mbb_set_limits(mbb_ctx *c, const double lowlim[5], const int32_t has_uplim[6],
                              const double uplim[6])
{
    if (!c || !lowlim || !has_uplim || !uplim) return fail(MBB_ERR_ARG, "null argument");
    c->has_uplim = 0;
    for (int i = 0; i < 5; ++i) c->lowlim[i] = lowlim[i];
    for (int i = 0; i < 6; ++i) {
        c->uplim[i] = has_uplim[i] ? uplim[i] : INFINITY;      // (a wall that is not set: never a NaN in the argument block)
        if (has_uplim[i]) c->has_uplim |= (1u << i);
    }
    return MBB_OK;
}

extern "C" int mbb_set_gpriors(mbb_ctx *c, const int32_t has[6], const double mean[6],
                               const double ivar[6])
{
    if (!c || !has || !mean || !ivar) return fail(MBB_ERR_ARG, "null argument");
    c->has_gprior = 0;
    for (int i = 0; i < 6; ++i) {
        c->gmean[i] = mean[i];
        c->givar[i] = ivar[i];
        if (has[i]) c->has_gprior |= (1u << i);
    }
    return MBB_OK;
}

// How mbb_lnlike_batch waits (option "spin_wait"): 0 blocks on the stream; 1 polls
// hipStreamQuery (measured on MI355X: no faster than 0); 2, the default for zero-copy
// batches of <= 8192 rows, watches the result slots in pinned host memory and falls back
// to 0 when they have not all appeared within "spin_budget" polls.
static const uint64_t kLnlSentinel = 0x7ff8dead5eed0001ull;
static const int32_t kStatusSentinel = 0x7fffff01;

static int wait_stream(mbb_ctx *c)
{
    if (c->opt.spin == 1) {
        for (;;) {
            hipError_t e = hipStreamQuery(c->stream);
            if (e == hipSuccess) return MBB_OK;
            if (e != hipErrorNotReady) return fail(MBB_ERR_HIP, "hipStreamQuery", e);
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

static int ensure_capacity(mbb_ctx *c, size_t n, bool want_flux)
{
    mbb_ctx::Boundary &b = c->bnd;
    int rc;
    if (n > b.cap) {
        size_t cap = b.cap ? b.cap : 256;
        while (cap < n) cap *= 2;
        // (grow() taken apart: the generation goes between the stream coming to rest and the first release)
        if ((rc = sync_stream(c))) return rc;
        // whoever holds addresses from mbb_boundary_buffers must see this BEFORE it writes through them again
        __atomic_store_n(&c->buf_gen, c->buf_gen + 1, __ATOMIC_RELEASE);
        b.cap = 0;
        c->call_in = nullptr; c->call_cap = 0;
        b.w_pars.release();
        if ((rc = b.d_pars.remake(cap * 5 * sizeof(double))) || (rc = b.d_lnl.remake(cap * sizeof(double))) ||
            (rc = b.d_status.remake(cap * sizeof(int32_t))) || (rc = b.h_pars.remake(cap * 5 * sizeof(double))) ||
            (rc = b.h_lnl.remake(cap * sizeof(double))) || (rc = b.h_status.remake(cap * sizeof(int32_t))))
            return rc;
        // With a large BAR the host can store into (fine-grained) device memory directly:
        // posted writes, and the kernel then reads its parameter rows from local memory
        // instead of pulling them across PCIe.
        if (c->large_bar < 0) {
            int lb = 0;
            if (hipDeviceGetAttribute(&lb, hipDeviceAttributeIsLargeBar, c->device) != hipSuccess) lb = 0;
            c->large_bar = lb;
        }
        // (refused: the rows go through the pinned block)
        if (c->large_bar > 0 && b.w_pars.remake(cap * 5 * sizeof(double))) (void)hipGetLastError();
        b.cap = cap;
    }
    if (want_flux && n * (size_t)c->nb > b.cap_flux) {
        size_t cap = b.cap * (size_t)c->nb;
        if (cap < n * (size_t)c->nb) cap = n * (size_t)c->nb;
        b.cap_flux = 0;
        if ((rc = grow(c, b.d_mflux, cap * sizeof(double))) || (rc = grow(c, b.h_mflux, cap * sizeof(double)))) return rc;
        b.cap_flux = cap;
    }
    return MBB_OK;
}

// LDS the kernel declares statically: the 2^(j/256) table and the piecewise polynomials
// (mbb_kernels.hip.h); the rest of the CU's 160 KB is what a launch may ask for dynamically.
static size_t static_lds(const mbb_ctx *c)
{
    return sizeof(double) * kExp2N + sizeof(double) * kPolyBDoubles +
           sizeof(double) * (c->opthin ? 2 : kPolyCDoubles);
}
static size_t dynamic_lds_limit(const mbb_ctx *c) { return 160 * 1024 - static_lds(c) - 2048; }
// The model variant, the first index of every kernel table: (opthin ? 2 : 0) | (noalpha ? 1 : 0)
static int model_of(const mbb_ctx *c) { return (c->opthin ? 2 : 0) | (c->noalpha ? 1 : 0); }

// Dynamic LDS of a k_lnlike workgroup of `wpb` walkers, without the staged passband tables and without
// the inverse covariance.
static size_t lnlike_lds_base(const mbb_ctx *c, int wpb)
{
    return (size_t)wpb * (sizeof(WalkerK) + 8 * (size_t)c->npart + 8 * (size_t)c->nb + 16) +
           16 * (size_t)c->nb + 8 * ((size_t)c->nb + 2) + 64 * (size_t)wpb;
}

// Walkers per workgroup and workgroup size.  mid_staged: the launch is of the middle regime below and
// wants its passband tables in LDS.
static void pick_geometry(const mbb_ctx *c, int n, int &wpb, int &threads, bool *mid_staged = nullptr)
{
    if (mid_staged) *mid_staged = false;
    // Small batches (an emcee half-step) are latency bound: one walker per
    // workgroup with about one segment per wave, so the chip sees n workgroups.
    // The static tables (36-57 KB) allow two workgroups per CU, so beyond one walker
    // per CU the workgroups are 512 threads wide -- 16 waves per CU -- and share their
    // tables among up to 32 walkers (a wave then takes whole walkers, 4 each).
    const long cus = c->cu_count;
    long w = 1, t = 256;
    if (n <= cus) {
        t = (long)((c->nunit + 3) / 4) * 256;          // ~ one unit per wave
        if (t > 1024) t = 1024;
        if (c->nunit <= 4) t = 256;
    } else {
        w = (n + cus * 2 - 1) / (cus * 2);
        if (w > 32) w = 32;
        t = 512;
        // The middle regime, more than one walker per CU but at most 256 (round 3, tools/sweep_geometry.py,
        // profiles/r03/geometry_sweep.txt): ONE workgroup of 1024 threads per CU with the passband tables
        // staged in LDS once for all its walkers beats two narrower workgroups reading them through L2 by
        // 13-17 % from 500 to 8192 rows, 7 % at 32768, 3 % at 65536; at 250 000 rows it is 3 % behind.
        const long wm = std::min<long>(64, (n + cus - 1) / cus);
        const size_t tables = (size_t)c->nchunk * 64 * 3 * sizeof(double);
        if (n <= 256 * cus && c->opt.wpb <= 0 && c->opt.threads <= 0 && c->opt.stage != 0 &&
            lnlike_lds_base(c, (int)wm) + (c->has_cov ? 8 * (size_t)c->nb * c->nb : 0) + tables + 16 <= dynamic_lds_limit(c)) {
            w = wm; t = 1024;
            if (mid_staged) *mid_staged = true;
        }
    }
    if (c->opt.wpb > 0) w = c->opt.wpb > 64 ? 64 : c->opt.wpb;
    wpb = (int)w;
    if (c->opt.threads > 0) t = c->opt.threads;
    if (t < 64) t = 64;
    if (t > 1024) t = 1024;
    threads = (int)((t / 64) * 64);
    // the prologue runs on one row of 16 lanes per walker
    if (threads < 16 * wpb) threads = ((16 * wpb + 63) / 64) * 64;
}

// Look-ahead sampler runs: how the workgroups that work ahead are shaped.  One row of 16 lanes per candidate proposal
// -- 4 per walker of a half: a row keeps to one half (SMODE 6) -- `rows` of them per wave, `aw` such waves per workgroup.
// A constructor is one dependent chain and a wave alone on its SIMD runs it fastest, so the candidates are spread as
// thinly as the CUs the movers leave free allow.  Where even the densest packing (64 candidates per workgroup) leaves
// them too few, the run takes the launch train (plan_sampler_run); measured, the one-launch run is slower than the train
// there anyway (480 walkers: 17.7 against 15.8 us per step; 450 walkers, 32 per workgroup: 15.0 against 15.8 --
// profiles/r03/walker_sweep.txt).
static void lookahead_plan(const mbb_ctx *c, int movers, int threads, int half, int &rows, int &aw, int &n_ahead)
{
    const int pairs = 4 * half, free_cus = c->cu_count - movers;
    static const int plan[5][2] = {{1, 4}, {2, 4}, {4, 4}, {4, 8}, {4, 16}};
    rows = 1; aw = 4;
    for (int i = 0; i < 5; ++i) {
        rows = plan[i][0]; aw = std::min(plan[i][1], threads / 64);
        if ((pairs + rows * aw - 1) / (rows * aw) <= free_cus) break;
    }
    n_ahead = (pairs + rows * aw - 1) / (rows * aw);
}

constexpr long kFlowStrikes = 3, kFlowRest = 16;
constexpr long kServeRest = 4096;            // boundary calls the served path rests for after three lost servers in a row
static std::atomic<unsigned long long> g_flow_serial{0};   // one-launch sampler runs started in this process (their check words)

// One launch of the kernel in `slot` (kernel_slot): the module-launch entry with the argument block handed over as ONE
// packed buffer -- no per-argument marshalling in the runtime, 0.2 us per call less than hipLaunchKernel (A/B:
// tools/probe_boundary_breakdown.py, profiles/r04/boundary_breakdown.txt).  ev: null, or two events to record right
// before and right behind the launch.
static int launch_packed(mbb_ctx *c, int slot, int grid, int threads, size_t smem, LikeArgs &a, hipEvent_t *ev)
{
    void (*const kern)(const LikeArgs) = g_kernel[slot];
    if (static_lds(c) + smem > 60 * 1024) {
        // beyond 64 KB of LDS per workgroup (static + dynamic) the kernel's dynamic-LDS
        // ceiling has to be raised: once per context, variant and size, not per launch
        size_t &g = c->lds_granted[slot];
        if (smem > g) {
            const size_t dyn_limit = dynamic_lds_limit(c);
            size_t want = (smem + 16383) & ~(size_t)16383;
            if (want > dyn_limit) want = dyn_limit;
            HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
            g = want;
        }
    }
    hipFunction_t &f = c->mod_fn[slot];
    if (!f) HIPCHK(hipGetFuncBySymbol(&f, (const void *)kern));
    size_t sz = sizeof(a);
    void *extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
    // (hipExtModuleLaunchKernel would take the two events with the launch -- the dispatch's own timestamps, no marker
    // packets: measured, it costs 8 us MORE of host time per timed region than two hipEventRecord around the launch,
    // profiles/r04/timed_region.txt)
    if (ev) HIPCHK(hipEventRecord(ev[0], c->stream));
    HIPCHK(hipModuleLaunchKernel(f, (unsigned)grid, 1, 1, (unsigned)threads, 1, 1, (unsigned)smem, c->stream, nullptr, extra));
    if (ev) HIPCHK(hipEventRecord(ev[1], c->stream));
    return MBB_OK;
}

// The part of the argument block every kernel of the family reads alike: model, bands, data, limits and priors.
static void fill_model_args(const mbb_ctx *c, LikeArgs &a)
{
    a.nu = c->band.nu.d(); a.lnnu = c->band.lnnu.d(); a.wt = c->band.wt.d();
    a.poly_b = c->d_poly_b; a.poly_c = c->d_poly_c;
    a.unit_tab = c->band.unit_tab.d(); a.band_rng = c->band.band_rng.d(); a.tail_slot = c->band.tail_slot.d();
    a.flux = c->data.flux.d(); a.ivar = c->data.ivar.d(); a.invcov = c->has_cov ? c->data.invcov.d() : nullptr;
    a.nb = c->nb; a.nunit = c->nunit; a.npart = c->npart; a.nchunk = c->nchunk;
    a.nunorm = kUmToGHz / c->wavenorm;
    a.lnunorm = log(a.nunorm);
    for (int i = 0; i < 5; ++i) a.lowlim[i] = c->lowlim[i];
    for (int i = 0; i < 6; ++i) { a.uplim[i] = c->uplim[i]; a.gmean[i] = c->gmean[i]; a.givar[i] = c->givar[i]; }
    a.has_uplim = c->has_uplim; a.has_gprior = c->has_gprior;
    a.debug = (int)c->opt.debug;
#ifdef MBB_STAMPS
    a.stamps = c->stamps.d();
#endif
}

// What a k_lnlike launch of n walkers -- of given rows (launch_rows) or of a sampler form (launch_sampler) -- is shaped
// by: walkers per workgroup and workgroup size (pick_geometry), grid, dynamic LDS with the inverse covariance in it when
// that fits beside everything else, and the passband tables staged there too or not.  Fills the argument block but for
// what the kind of launch adds, and the launch's mbb_get_info "last_*" values.
struct LnlikeShape { int wpb, threads, grid; bool stage; size_t smem; };
static int lnlike_shape(mbb_ctx *c, int n, LnlikeShape &g, LikeArgs &a)
{
    bool mid_staged = false;
    pick_geometry(c, n, g.wpb, g.threads, &mid_staged);
    g.grid = (n + g.wpb - 1) / g.wpb;
    const size_t cov_bytes = c->has_cov ? 8 * (size_t)c->nb * c->nb : 0;
    const size_t smem_base = lnlike_lds_base(c, g.wpb);
    const size_t dyn_limit = dynamic_lds_limit(c);
    const bool cov_in_lds = c->has_cov && smem_base + cov_bytes <= std::min<size_t>(64 * 1024, dyn_limit);
    const size_t smem = smem_base + (cov_in_lds ? cov_bytes : 0);
    if (smem > dyn_limit) return fail(MBB_ERR_ARG, "band tables too large for the LDS plan");
    // LDS staging of the passband tables.  Measured (profiles/r01/ab_stage.txt, interleaved A/B): in the latency regime
    // (one walker per workgroup, the copy hides under the prologue) it is 1.5 % faster; with many walkers per workgroup it
    // is 4-5 % slower than reading the tables through L2, because 60 KB of LDS per workgroup caps residency at two per CU.
    const size_t table_bytes = (size_t)c->nchunk * 64 * 3 * sizeof(double);
    g.stage = ((g.wpb == 1 && n <= c->cu_count) || mid_staged) && smem + table_bytes + 16 <= dyn_limit;
    if (c->opt.stage == 0) g.stage = false;
    if (c->opt.stage == 1) g.stage = smem + table_bytes + 16 <= dyn_limit;
    g.smem = smem + (g.stage ? table_bytes + 16 : 0);
    if (c->nsrc > 1 && n % c->nsrc != 0) return fail(MBB_ERR_ARG, "row count must be a multiple of the number of sources");
    memset(&a, 0, sizeof a);
    fill_model_args(c, a);
    a.n = n; a.wpb = g.wpb; a.cov_in_lds = cov_in_lds ? 1 : 0; a.nsrc = c->nsrc;
    a.rows_per_src = c->nsrc > 1 ? n / c->nsrc : 0;
    a.stretch_a = 2.0; a.zpow = 4.0;
    c->last_wpb = g.wpb; c->last_threads = g.threads; c->last_grid = g.grid; c->last_smem = (long)g.smem;
    c->last_stage = g.stage ? 1 : 0; c->last_prepass = 0;
    return MBB_OK;
}

// The likelihood of n given rows: k_lnlike SMODE 0, after k_walker_pre for big batches
static int launch_rows(mbb_ctx *c, const double *d_pars, int n, double *d_lnl, int32_t *d_status, double *d_mflux)
{
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    if (c->data_nb != c->nb) return fail(MBB_ERR_STATE, "data not set or band count mismatch");
    if (n <= 0) return MBB_OK;
    LnlikeShape g;
    LikeArgs a;
    int rc = lnlike_shape(c, n, g, a);
    if (rc) return rc;
    a.pars = d_pars; a.lnl = d_lnl; a.status = d_status; a.model_flux = d_mflux;
    // Big batches of given rows: gate, constructor and penalties by a pass of their own with a LANE per walker (k_walker_pre)
    // -- where a launch is bound by the number of instructions it issues, a row of 16 lanes per walker spends a quarter of
    // them on the constructors (cfg5's 250 000 rows: 1.31 -> 1.0x ms).  Option "prepass": -1 auto (from 64 walkers per CU),
    // 0 never, 1 always.
    if (c->opt.prepass > 0 || (c->opt.prepass < 0 && (long)n >= 64L * c->cu_count)) {
        const size_t need = (size_t)n * kPreWords * sizeof(double);
        size_t cap = c->pre.cap ? c->pre.cap : 16384 * (size_t)kPreWords * sizeof(double);
        while (cap < need) cap *= 2;
        if ((rc = grow(c, c->pre, cap))) return rc;
        a.spec = c->pre.d();
        static void (*const ptable[4])(const LikeArgs) = {k_walker_pre<false, false>, k_walker_pre<false, true>,
                                                          k_walker_pre<true, false>, k_walker_pre<true, true>};
        hipLaunchKernelGGL(ptable[model_of(c)], dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
        HIPCHK(hipGetLastError());
        c->last_prepass = 1;
    }
    c->last_smode = 0; c->last_ahead = 0;
    return launch_packed(c, kernel_slot(kLnlike, model_of(c), g.stage ? 1 : 0), g.grid, g.threads, g.smem, a, nullptr);
}

extern "C" int mbb_lnlike_batch_device(mbb_ctx *c, const double *d_pars, int n, double *d_lnl,
                                       int32_t *d_status, double *d_mflux)
{
    int rc = use(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_pars || !d_lnl))) return fail(MBB_ERR_ARG, "bad batch buffers");
    return launch_rows(c, d_pars, n, d_lnl, d_status, d_mflux);
}

extern "C" int mbb_lnlike_repeat_device(mbb_ctx *c, const double *d_pars, int n, double *d_lnl,
                                        int32_t *d_status, int reps)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || reps <= 0 || !d_pars || !d_lnl) return fail(MBB_ERR_ARG, "bad batch buffers");
    for (int r = 0; r < reps; ++r)
        if ((rc = launch_rows(c, d_pars, n, d_lnl, d_status, nullptr))) return rc;
    return MBB_OK;
}

// The zero-copy host path once the parameter rows are where the kernel reads them (device memory the host
// wrote through the BAR when `push`, the pinned block otherwise): launch, watch the result slots in pinned
// memory (or wait for the stream), leave lnl / status / model flux in the boundary's pinned blocks (c->bnd.h_lnl, h_status, h_mflux).
static int lnlike_zero_copy(mbb_ctx *c, int n, bool push, bool model_flux, long t_a)
{
    int rc;
    auto now_ns = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1000000000L + ts.tv_nsec; };
    // the kernel reads the pinned parameter block and writes lnL straight
    // into pinned host memory: no copy commands on the stream at all
    double *const dp = push ? c->bnd.w_pars.d() : c->bnd.h_pars.dv(), *const dl = c->bnd.h_lnl.dv(), *const df = model_flux ? c->bnd.h_mflux.dv() : nullptr;
    int32_t *const ds = c->bnd.h_status.dv();
    // spin_wait = 2: do not wait for the kernel's completion signal at all.  The
    // result slots in pinned memory are pre-filled with patterns the kernel never
    // writes (a NaN with a payload; it produces the canonical NaN), and the host
    // watches them: a walker's results are final the moment they appear, before the
    // end-of-kernel bookkeeping.  status is written after lnl by the same lane.
    const bool watch = c->opt.spin == 2 && !model_flux && n <= 8192;
    c->last_watch_seen = -1;
    if (watch) {
        uint64_t *hl = reinterpret_cast<uint64_t *>(c->bnd.h_lnl.h());
        for (int i = 0; i < n; ++i) { hl[i] = kLnlSentinel; c->bnd.h_status.h()[i] = kStatusSentinel; }
    }
    const long t_b = now_ns();
    if ((rc = launch_rows(c, dp, n, dl, ds, df))) return rc;
    const long t_c = now_ns();
    bool seen = false;
    if (watch) {
        // acquire loads: the copies out of h_lnl / h_status below must not be satisfied
        // from before the slot was seen to change
        const uint64_t *hl = reinterpret_cast<const uint64_t *>(c->bnd.h_lnl.h());
        const int32_t *hs = c->bnd.h_status.h();
        int i = 0;
        for (long spins = 0; spins < c->opt.spin_budget; ++spins) {   // default ~ tens of ms, then give up
            while (i < n && __atomic_load_n(&hl[i], __ATOMIC_ACQUIRE) != kLnlSentinel &&
                   __atomic_load_n(&hs[i], __ATOMIC_ACQUIRE) != kStatusSentinel) ++i;
            if (i == n) { seen = true; break; }
            __builtin_ia32_pause();
        }
        c->last_watch_seen = seen ? 1 : 0;
    }
    if (!seen && (rc = wait_stream(c))) return rc;
    c->t_prep_ns = t_b - t_a; c->t_launch_ns = t_c - t_b; c->t_wait_ns = now_ns() - t_c;
    return MBB_OK;
}

extern "C" int mbb_lnlike_batch(mbb_ctx *c, const double *pars, int n, double *lnl,
                                int32_t *status, double *model_flux)
{
    int rc = use(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!pars || !lnl))) return fail(MBB_ERR_ARG, "bad batch buffers");
    if (n == 0) return MBB_OK;
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    if ((rc = ensure_capacity(c, (size_t)n, model_flux != nullptr))) return rc;
    const size_t nbytes = (size_t)n * 5 * sizeof(double);
    auto now_ns = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1000000000L + ts.tv_nsec; };
    const long t_a = now_ns();
    const bool push = c->opt.zero_copy && c->opt.bar_params && c->bnd.w_pars.d();
    if (push) {
        memcpy(c->bnd.w_pars.d(), pars, nbytes);           // CPU stores through the BAR ...
        __builtin_ia32_sfence();                   // ... drained before the doorbell is rung
    } else {
        memcpy(c->bnd.h_pars.h(), pars, nbytes);
    }
    if (c->opt.zero_copy) {
        if ((rc = lnlike_zero_copy(c, n, push, model_flux != nullptr, t_a))) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(c->bnd.d_pars.d(), c->bnd.h_pars.h(), nbytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = launch_rows(c, c->bnd.d_pars.d(), n, c->bnd.d_lnl.d(), c->bnd.d_status.d(),
                                model_flux ? c->bnd.d_mflux.d() : nullptr))) return rc;
        HIPCHK(hipMemcpyAsync(c->bnd.h_lnl.h(), c->bnd.d_lnl.d(), (size_t)n * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->bnd.h_status.h(), c->bnd.d_status.d(), (size_t)n * sizeof(int32_t),
                              hipMemcpyDeviceToHost, c->stream));
        if (model_flux)
            HIPCHK(hipMemcpyAsync(c->bnd.h_mflux.h(), c->bnd.d_mflux.d(), (size_t)n * c->nb * sizeof(double),
                                  hipMemcpyDeviceToHost, c->stream));
        if ((rc = wait_stream(c))) return rc;
    }
    memcpy(lnl, c->bnd.h_lnl.h(), (size_t)n * sizeof(double));
    if (status) memcpy(status, c->bnd.h_status.h(), (size_t)n * sizeof(int32_t));
    if (model_flux) memcpy(model_flux, c->bnd.h_mflux.h(), (size_t)n * c->nb * sizeof(double));
    return MBB_OK;
}

// The boundary call with the copies taken out (the caller is likelihood.__call__,
// likelihood.py:790-834, once per emcee half-step).  mbb_boundary_buffers hands the binding the host
// addresses of the block it writes the parameter rows INTO -- device memory behind the BAR where there is one,
// else the pinned block the kernel reads -- and of the pinned blocks the kernel writes lnprob and row status
// to; mbb_lnlike_call then evaluates the first n rows of that block: no pointer arguments, no memcpy on either
// side, the row status looked through here.  The addresses hold until a call asks for more rows than `nmax`
// (ask again then) or the context is destroyed.
extern "C" const unsigned long long *mbb_boundary_generation(mbb_ctx *c)
{
    return c ? &c->buf_gen : nullptr;
}

extern "C" int mbb_boundary_buffers(mbb_ctx *c, int nmax, double **in, double **out, int32_t **status)
{
    int rc = use(c);
    if (rc) return rc;
    if (nmax <= 0 || !in || !out) return fail(MBB_ERR_ARG, "bad arguments");
    if ((rc = ensure_capacity(c, (size_t)nmax, false))) return rc;
    const bool push = c->opt.zero_copy && c->opt.bar_params && c->bnd.w_pars.d();
    c->call_in = push ? c->bnd.w_pars.d() : c->bnd.h_pars.h();
    c->call_cap = c->bnd.cap;
    *in = c->call_in; *out = c->bnd.h_lnl.h();
    if (status) *status = c->bnd.h_status.h();
    return MBB_OK;
}

// ---- the served boundary ----------------------------------------------------------------------------------------
// (see mbb_serve.hip.h for what it is and why)
// Called with c->srv_mu held (by c's owner, or by a visiting sibling: yield_server).
static int serve_stop(mbb_ctx *c)
{
    if (!c->serving) return MBB_OK;
    c->serving = false;
    if (c->device >= 0 && c->device < 64) {
        std::lock_guard<std::mutex> lk(g_dev_mutex);
        if (g_dev[c->device].server == c) g_dev[c->device].server = nullptr;
    }
    // a request number the server has not seen, with the row count that means "leave"
    __atomic_store_n(c->srv.w_door.d(), (++c->srv_seq << 16) | kServeQuit, __ATOMIC_RELAXED);
    __builtin_ia32_sfence();
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

// Start a server with the request in the launch itself.  The argument block is launch_rows', filled in here for
// the fields k_serve reads.
// How many workgroups a server of this context is started with: a row each for the widest call so far, in eights -- not
// one per CU: what it does not hold is there for the launches and the servers of other processes (two pool workers of 125
// rows each have their servers side by side, 8.7 us per call in both: profiles/r05/pool_two_processes_sized.txt) --, and never
// more than this process's share of the device.
static int serve_grid(const mbb_ctx *c, int n, int share)
{
    int g = c->opt.serve_grid > 0 ? (int)c->opt.serve_grid : std::max(c->srv_want, (n + 7) & ~7);
    return std::min(std::min(g, share), c->cu_count);
}

// (the launch itself; serve_start below claims the device around it)
static int serve_launch(mbb_ctx *c, int n, unsigned long long word, int grid)
{
    if (!c->srv.w_door.p && c->srv.w_door.remake(64)) {
        (void)hipGetLastError();                   // (no fine-grained memory to be had: every call is a launch)
        return 1;
    }
    if (!c->srv.h_gone.p)
        if (const int rc = c->srv.h_gone.remake(64)) return rc;

    LikeArgs a;
    memset(&a, 0, sizeof a);
    fill_model_args(c, a);
    a.pars = c->bnd.w_pars.d(); a.n = n; a.lnl = c->srv.h_srv.dv(); a.status = nullptr; a.model_flux = nullptr;
    a.wpb = 1; a.nsrc = 1;
    int wpb, threads;
    pick_geometry(c, 1, wpb, threads);
    const size_t dyn_limit = dynamic_lds_limit(c);
    const size_t table_bytes = (size_t)c->nchunk * 64 * 3 * sizeof(double);
    a.cov_in_lds = (c->has_cov && serve_lds(c->nb, c->npart, true) <= std::min<size_t>(64 * 1024, dyn_limit)) ? 1 : 0;
    const size_t sm = serve_lds(c->nb, c->npart, a.cov_in_lds != 0);
    const bool stg = c->opt.stage != 0 && sm + table_bytes + 16 <= dyn_limit;
    // The quadrature beside the constructor (mbb_serve.hip.h): every wave but the first keeps both candidates of its own
    // unit's samples in registers
    // -- with a chunk of samples at least for each of twelve waves: with fewer the extra barrier costs more than there is to
    // gain (cfg1's one chunk: 8.5-8.7 -> 8.9 us per 25-row call; option "serve_overlap" 2: regardless; 0: never)
    // -- and waves to work ahead with (a workgroup narrowed by option "block_threads" may have none besides the constructor's)
    // -- and units of at most four chunks (option "seg_chunks")
    const bool ovl = c->opt.serve_overlap != 0 && (c->nchunk >= 12 || c->opt.serve_overlap == 2) && threads >= 256 &&
                     c->opt.seg_chunks >= 1 && c->opt.seg_chunks <= 4;
    a.spec_cfg = ovl ? 1 : 0;
    const size_t sm_total = sm + (stg ? table_bytes + 16 : 0);
    if (sm_total > dyn_limit) return 1;
    a.chain6 = reinterpret_cast<double *>(c->srv.h_gone.dv());
    a.pos6 = reinterpret_cast<double *>(c->srv.w_door.d());
    a.seed = word;
    a.persist = (int)std::min<long>(std::max<long>(c->opt.serve_idle_us, 20), 1000000);
    *c->srv.h_gone.h() = 0;
    __atomic_store_n(c->srv.w_door.d(), word, __ATOMIC_RELAXED);
    __builtin_ia32_sfence();
    {
        int rc = launch_packed(c, kernel_slot(kServe, model_of(c), (ovl ? 2 : 0) + (stg ? 1 : 0)), grid, threads, sm_total, a,
                               nullptr);
        if (rc) return rc;
    }
    c->srv_grid = grid;
    c->last_wpb = 1; c->last_threads = threads; c->last_grid = grid; c->last_smem = (long)sm_total;
    c->last_stage = stg ? 1 : 0; c->last_smode = 10;
    c->serving = true;
    c->srv_run = 0;
    { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); c->srv_t0_ns = ts.tv_sec * 1000000000L + ts.tv_nsec; }
    return MBB_OK;                                 // (the device has had this context's name since the claim above)
}

// Starts a resident server for this context.  The device is CLAIMED before anything is launched: two contexts on two
// threads that both found no server resident (yield_server) would otherwise both start one, the device would remember
// the second, and nobody could find the first to tell it to leave.  Whoever comes second sends its rows by
// a launch (1); its next call finds the first's server by name and tells it to go.
static int serve_start(mbb_ctx *c, int n, unsigned long long word, int grid)
{
    if (grid <= 0 || n > kServePasses * grid) return 1;
    const bool named = c->device >= 0 && c->device < 64;
    if (named) {
        std::lock_guard<std::mutex> lk(g_dev_mutex);
        mbb_ctx *&sv = g_dev[c->device].server;
        if (sv && sv != c) return 1;
        sv = c;
    }
    const int rc = serve_launch(c, n, word, grid);
    if (rc != MBB_OK && named) {
        std::lock_guard<std::mutex> lk(g_dev_mutex);
        if (g_dev[c->device].server == c) g_dev[c->device].server = nullptr;
    }
    return rc;
}

// One request: MBB_OK when the results are in the pinned slots, 1 when the rows have to go by a launch after all,
// negative on error.  The parameter rows are in c->bnd.w_pars already.
static int serve_request(mbb_ctx *c, int n, int grid)
{
    const int kPfAhead = (int)c->opt.serve_prefetch;
    auto now_ns = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1000000000L + ts.tv_nsec; };
    const long t_a = now_ns();
    // (the records exist once a server has been started; before that serve_start makes them)
    if (!c->srv.h_srv.p)
        if (const int rc = c->srv.h_srv.remake((size_t)kServePasses * c->cu_count * 8 * kSrvStride)) return rc;
    uint64_t *hr = reinterpret_cast<uint64_t *>(c->srv.h_srv.h());
    for (int i = 0; i < n; ++i) hr[kSrvStride * i + 1] = (uint64_t)kStatusSentinel;
    const unsigned long long word = (++c->srv_seq << 16) | (unsigned long long)n;
    __builtin_ia32_sfence();                       // the caller's rows, through the BAR, before the request
    const long t_b = now_ns();
    long budget_ns = c->opt.serve_budget_us * 1000L;
    if (!c->serving) {
        int rc = serve_start(c, n, word, grid);
        if (rc) return rc;
        budget_ns += 200000L;                      // (a launch, and the tables into LDS on every CU)
    } else {
        __atomic_store_n(c->srv.w_door.d(), word, __ATOMIC_RELAXED);
        __builtin_ia32_sfence();
    }
    const long t_c = now_ns();
    ++c->srv_requests;
    int i = 0;
    bool seen = false;
    for (long spins = 0;; ++spins) {
        // a record is one 16-byte store: when its status word has turned, its lnl is there
        while (i < n && __atomic_load_n(&hr[kSrvStride * i + 1], __ATOMIC_ACQUIRE) != (uint64_t)kStatusSentinel) {
            // (the GPU's writes took the records' lines out of this core's caches: once the first has turned the others are
            // landing, and their misses are asked for kPfAhead lines ahead of the scan instead of one by one behind it --
            // tools/lat_doorbell.hip: the scan of 125 landed lines 0.67-1.29 -> 0.65-0.76 us.  Not before the first has
            // turned: a line that sits in the core's cache when the GPU wants to write it costs the GPU a snoop)
            if (i == 0) for (int k = 1; k < kPfAhead && k < n; ++k) __builtin_prefetch(&hr[kSrvStride * k], 0, 3);
            if (kPfAhead && i + kPfAhead < n) __builtin_prefetch(&hr[kSrvStride * (i + kPfAhead)], 0, 3);
            c->bnd.h_lnl.h()[i] = c->srv.h_srv.h()[kSrvStride * i];
            c->bnd.h_status.h()[i] = (int32_t)hr[kSrvStride * i + 1];
            ++i;
        }
        if (i == n) { seen = true; break; }
        if ((spins & 63) == 63 && (now_ns() - t_c > budget_ns || __atomic_load_n(c->srv.h_gone.h(), __ATOMIC_ACQUIRE) != 0)) break;
        __builtin_ia32_pause();
    }
    c->last_watch_seen = seen ? 1 : 0;
    c->t_prep_ns = t_b - t_a; c->t_launch_ns = t_c - t_b; c->t_wait_ns = now_ns() - t_c;
    if (seen) {
        c->srv_strikes = 0;
        if (++c->srv_run >= 256) c->srv_need = 0;
        return MBB_OK;
    }
    // the records did not turn: the server had left when the request came (it says so: nothing wrong, the sampler's
    // calls were further apart than its patience), or it was leaving, or it is not resident.  It is told to go, waited
    // for, and the rows go by a launch; three requests in a row lost to a server that had NOT said it was gone, and
    // the feature rests for the next kServeRest boundary calls (rounds 4-5: for the life of the context -- one bad
    // stretch on a shared box, and a sampler's every later call was a launch; the sampler forms rest the same way).
    ++c->srv_fallbacks;
    c->srv_hot = 0;
    if (__atomic_load_n(c->srv.h_gone.h(), __ATOMIC_ACQUIRE) == 0 && ++c->srv_strikes >= 3) {
        c->srv_strikes = 0;
        c->srv_rest = kServeRest;
        ++c->srv_rests;
    }
    int rc = serve_stop(c);
    return rc ? rc : 1;
}

// Returns MBB_OK, a negative error, or -- positive -- the status code of the first row that the reference
// would have raised for (alpha <= 0, beta < 0, no merge point: modified_blackbody.py:219-224, :294-316).
extern "C" int mbb_lnlike_call(mbb_ctx *c, int n)
{
    if (!c) return fail(MBB_ERR_ARG, "null context");
    HIPCHK(hipSetDevice(c->device));               // (not use(): a resident server stays, the streak of calls goes on)
    std::lock_guard<std::mutex> own(c->srv_mu);    // (uncontended: ~20 ns; a sibling's visit waits for the call to end)
    int rc;
    if (n <= 0) return n == 0 ? MBB_OK : fail(MBB_ERR_ARG, "bad row count");
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    const bool push = c->opt.zero_copy && c->opt.bar_params && c->bnd.w_pars.d();
    if (!c->opt.zero_copy || !c->call_in || c->call_cap != c->bnd.cap || (size_t)n > c->bnd.cap ||
        c->call_in != (push ? c->bnd.w_pars.d() : c->bnd.h_pars.h())) {
        if (c->serving && (rc = serve_stop(c))) return rc;
        return fail(MBB_ERR_STATE, "mbb_boundary_buffers first (or again: the buffers or the host-path options changed)");
    }
    // After a few boundary calls in a row with nothing else in between -- a sampler's loop -- the rows are handed to
    // a kernel that stays on the GPU (k_serve) instead of a launch each: while the batch is at most a row per CU and the
    // host path is the default one.  One server per device and process: whichever context comes to the device tells a
    // sibling's to leave first (use(), and the line below).
    bool can_serve = c->opt.serve && push && n <= kServePasses * c->cu_count && c->nsrc <= 1 && c->opt.spin == 2 && c->data_nb == c->nb;
    if (c->srv_rest > 0) { --c->srv_rest; can_serve = false; }      // (resting after three lost servers in a row)
    // ... and across PROCESSES (emcee's pool, mbb_fit.py:80-81 threads > 1: the likelihood pickled into workers that share the
    // GPU): a server holds a CU per workgroup, and nothing of another process fits on those -- with round 4's server on every
    // CU one worker's call waited 42 ms for the other's whole loop (profiles/r05/pool_two_processes_before.txt).  So a server is
    // as wide as the calls have rows, and no wider than this process's share of the device: the CUs divided by the processes
    // of this library that are making boundary calls on it right now (csrc/mbb_registry.h: each says so at every call; one
    // that holds a context but does not call -- a pool's parent -- is not in the way).  A call of more rows than the share goes
    // by a launch; a server that is too wide for the share, or too narrow for the call, leaves and the next starts with this
    // call.  ("serve" 2: the whole device is this process's share -- tests.)
    int share = c->cu_count, grid = 0;
    const long need_hot = c->srv_need > 0 ? c->srv_need : c->opt.serve_after;
    timespec tb = {0, 0};
    if (can_serve) {
        clock_gettime(CLOCK_MONOTONIC, &tb);                   // (one look at the clock: who is busy, and the lease)
        if (c->opt.serve != 2) {
            const uint64_t now_ms = (uint64_t)tb.tv_sec * 1000u + (uint64_t)(tb.tv_nsec / 1000000);
            // (before a server is there every call looks: a pool's workers begin together, and three servers of 128 do not fit)
            const int busy = mbbh::registry_busy(c->reg_key, now_ms, 250, !c->serving);
            // (the dispatcher deals a kernel's workgroups to the device's 8 XCDs in turn, and there they stay: what has to fit
            // is every process's ceil(workgroups / 8) into an XCD's CUs -- three servers of 85 are 33 on the first XCDs of 32,
            // one workgroup never starts and every request of its server times out)
            share = c->xcds * ((c->cu_count / c->xcds) / (busy + 1));
            c->srv_busy = busy;
        }
        c->srv_want = std::max(c->srv_want, std::min((n + 7) & ~7, c->cu_count));
        grid = serve_grid(c, n, share);
        // (a server narrower than the call has rows takes them in turns, kServePasses rows a workgroup at most: beyond that a
        // launch is the faster way)
        if (grid <= 0 || n > kServePasses * grid) {
            // (counted once per run of calls that would have been served)
            if (c->serving || ++c->srv_hot == need_hot) ++c->srv_peer_yields;
            can_serve = false;
        } else if (c->serving && (c->srv_grid > share || (n > c->srv_grid && grid > c->srv_grid))) {
            if ((rc = serve_stop(c))) return rc;
            c->srv_hot = need_hot;
            ++c->srv_resizes;
        }
    }
    // ... and not for ever in one go: processes the registry cannot see get the CUs when the lease is up (the rows of this
    // call go by a launch, a new server starts after the next few calls in a row)
    if (can_serve && c->serving && c->opt.serve_lease_us > 0) {
        if (tb.tv_sec * 1000000000L + tb.tv_nsec - c->srv_t0_ns > c->opt.serve_lease_us * 1000L) {
            can_serve = false;
            c->srv_hot = 0;
            ++c->srv_lease_yields;
        }
    }
    // (a sibling context's server: this call, served or launched, needs the CUs; and a sibling's visit in between ends this
    // context's run of calls)
    if (!c->serving && (rc = yield_server(c))) return rc;
    bool done = false;
    if (can_serve && (c->serving || ++c->srv_hot >= need_hot)) {
        rc = serve_request(c, n, grid);
        if (rc < 0) return rc;
        done = rc == MBB_OK;
    } else if (c->serving && (rc = serve_stop(c))) {
        return rc;
    }
    if (!done) {
        timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
        if (push) __builtin_ia32_sfence();         // the caller's stores through the BAR, drained before the doorbell
        if ((rc = lnlike_zero_copy(c, n, push, false, ts.tv_sec * 1000000000L + ts.tv_nsec))) return rc;
    }
    const int32_t *hs = c->bnd.h_status.h();
    for (int i = 0; i < n; ++i)
        if (hs[i] >= 2 && hs[i] != 7) return hs[i];
    return MBB_OK;
}

// ---- device-resident ensemble sampler ----------------------------------------
constexpr size_t kChainDirectBytes = (size_t)8 << 20;   // stored chains up to this size go straight into the caller's arrays
struct mbb_sampler_state : mbbo::SamplerMem {      // (its device and pinned memory: mbb_owned.h)
    int nw = 0;            // walkers per source
    int nsrc = 1;          // independent ensembles advanced together
    bool backup_kept = false;            // the last run kept d_bak, a copy of what it started from to redo it from
    bool unchecked = false;              // an asynchronous advance was enqueued and its error flag not looked at yet
    bool lost = false;                   // such an advance gave up: the rows are no state of the chain until set again
    int spec_form = 0;                   // the sampler form whose state d_spec holds (0: none / not to be trusted)
    int flowm_parity = 0;                // form 7: the set of completion counters the next launch uses
    size_t chain_cap = 0;                // doubles of d_chain6, and of d_chain_out
    bool h_chain_tried = false;          // the landing buffer was asked for since d_chain_out was last made
    int resident_nsteps = 0;             // steps of the chain d_chain_out holds in the caller's layout (0: none)
    unsigned long long seed = 0, steps_done = 0;
    double zpow = 4.0;                   // the exponent of z in the accept test: (columns the ensemble spans) - 1, set_state
    int rows() const { return nw * nsrc; }
};

extern "C" int mbb_sampler_create(mbb_ctx *c, int nwalkers, unsigned long long seed, void **out)
{
    int rc = use(c);
    if (rc) return rc;
    if (!out || nwalkers < 2 || (nwalkers & 1)) return fail(MBB_ERR_ARG, "nwalkers must be even");
    std::unique_ptr<mbb_sampler_state> s(new mbb_sampler_state());
    s->nw = nwalkers;
    s->nsrc = c->nsrc > 0 ? c->nsrc : 1;
    s->seed = seed;
    const size_t R = (size_t)s->rows();
    if (c->x.connected) {
        // sharded with the one-hop exchange: the ensemble lives where the peers can write it
        if (R > c->x.cap_rows) return fail(MBB_ERR_ARG, "more walkers than the exchange buffer holds");
        s->d_pos6 = c->x.pos6(c->x.rank);
    } else {
        if ((rc = s->pos6_own.remake(R * 6 * sizeof(double)))) return rc;
        s->d_pos6 = s->pos6_own.d();
    }
    if ((rc = s->d_nacc.remake(R * sizeof(unsigned int))) || (rc = s->d_err.remake(sizeof(int)))) return rc;
    HIPCHK(hipMemset(s->d_nacc.d(), 0, R * sizeof(unsigned int)));
    HIPCHK(hipMemset(s->d_err.d(), 0, sizeof(int)));
    if (!s->pos6_own.p) ++c->x.users;       // (only a sampler that exists is counted: mbb_xchg_close waits for the count)
    *out = s.release();
    return MBB_OK;
}

extern "C" int mbb_sampler_destroy(mbb_ctx *c, void *sp)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s) return MBB_OK;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!s->pos6_own.p && c->x.users > 0) --c->x.users;
    delete s;
    return MBB_OK;
}

static int sampler_check_pending(mbb_ctx *c, mbb_sampler_state *s);

// The completion counters of a sampler's one-launch runs (forms 7 and 9; FlowMView's `done`), [2][ring][shards] as the
// kernels lay them out (mbb_flow_index.h), one value per counter: read (store 0) or written (store 1) with the stream
// idle.  *next_set is the set the sampler's next launch uses.  For the tests that hold the lag guard's bookkeeping.
extern "C" int mbb_sampler_flow_counters(mbb_ctx *c, void *sp, unsigned long long *counters, int cap, int store, int *ring,
                                         int *shards, int *next_set)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    const int n = 2 * kFmRing * kFmShards;
    if (!s || !counters || !ring || !shards || !next_set || cap < n) return fail(MBB_ERR_ARG, "bad arguments");
    if (!s->d_spec.p || (s->spec_form != 7 && s->spec_form != 9))
        return fail(MBB_ERR_STATE, "the sampler holds no state of a one-launch run (forms 7, 9)");
    HIPCHK(hipStreamSynchronize(c->stream));
    const FlowMView fv = flowm_view(s->d_spec.d(), s->rows());
    std::vector<unsigned long long> w(kFmDoneWords);
    HIPCHK(hipMemcpy(w.data(), fv.done, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int set = 0; set < 2; ++set)
        for (int slot = 0; slot < kFmRing; ++slot)
            for (int sh = 0; sh < kFmShards; ++sh) {
                unsigned long long &word = w[fm_done_word(set, slot, sh)], &val = counters[(set * kFmRing + slot) * kFmShards + sh];
                if (store) word = val;
                else val = word;
            }
    if (store) HIPCHK(hipMemcpy(fv.done, w.data(), w.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    *ring = kFmRing; *shards = kFmShards; *next_set = s->flowm_parity;
    return MBB_OK;
}

extern "C" int mbb_sampler_reset(mbb_ctx *c, void *sp)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s) return fail(MBB_ERR_ARG, "null sampler");
    (void)sampler_check_pending(c, s);       // (a give-up of an asynchronous advance is remembered, not wiped with the flag)
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemset(s->d_nacc.d(), 0, (size_t)s->rows() * sizeof(unsigned int)));
    HIPCHK(hipMemset(s->d_err.d(), 0, sizeof(int)));
    return MBB_OK;
}

// Set the ensemble(s): pos [nsrc][nw][5]; lnprob [nsrc][nw] or NULL (then evaluated
// on the device).  In a sharded run every rank sets the same, complete state.
extern "C" int mbb_sampler_set_state(mbb_ctx *c, void *sp, const double *pos, const double *lnprob)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s || !pos) return fail(MBB_ERR_ARG, "null argument");
    if (s->nsrc != c->nsrc) return fail(MBB_ERR_STATE, "number of sources changed since the sampler was made");
    const int R = s->rows();
    std::vector<double> lnp(R);
    if (lnprob) {
        for (int i = 0; i < R; ++i) lnp[i] = lnprob[i];
    } else {
        std::vector<int32_t> st(R);
        if ((rc = mbb_lnlike_batch(c, pos, R, lnp.data(), st.data(), nullptr))) return rc;
        for (int i = 0; i < R; ++i)
            if (st[i] >= 2) return fail(MBB_ERR_ARG, "initial position is not a valid SED or lnprob is NaN");
    }
    // The stretch move's Jacobian is z^(d - 1), d the dimension of the space the walkers span.  A column that is
    // constant over an ensemble stays so exactly (stretch_q with c == s), which is how a parameter is held fixed: d
    // counts the other columns, here, once per state.  One exponent per run: the sources must agree on which columns
    // are constant.  (Walkers on a tilted plane -- rank deficiency that is not axis-aligned -- are not looked for.)
    int nfree = 0;
    for (int src = 0; src < s->nsrc; ++src) {
        unsigned int mask = 0;
        const double *p0 = pos + (size_t)src * s->nw * 5;
        for (int w = 1; w < s->nw; ++w)
            for (int k = 0; k < 5; ++k)
                if (p0[(size_t)w * 5 + k] != p0[k]) mask |= 1u << k;
        const int nf = __builtin_popcount(mask);
        if (src > 0 && nf != nfree) return fail(MBB_ERR_ARG, "the sources' initial ensembles differ in the number of constant (fixed) columns");
        nfree = nf;
    }
    std::vector<double> rows((size_t)R * 6);
    for (int i = 0; i < R; ++i) {
        for (int k = 0; k < 5; ++k) rows[(size_t)i * 6 + k] = pos[(size_t)i * 5 + k];
        rows[(size_t)i * 6 + 5] = lnp[i];
        if (lnp[i] != lnp[i]) return fail(MBB_ERR_ARG, "initial lnprob is NaN");
    }
    HIPCHK(hipMemcpyAsync(s->d_pos6, rows.data(), rows.size() * sizeof(double),
                          hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (s->lost || s->unchecked) {
        // whatever an asynchronous advance left in the flag belongs to the state just replaced
        HIPCHK(hipMemset(s->d_err.d(), 0, sizeof(int)));
        s->lost = s->unchecked = false;
        s->spec_form = 0;
    }
    s->zpow = nfree > 1 ? (double)(nfree - 1) : 0.0;
    return MBB_OK;
}

// What an asynchronous advance left behind, looked at once before anything is built on it: a one-launch
// run that gave up (flag 9) kept no copy to be redone from, so the rows are not a state of the chain.  Without
// this look the next run would back those rows up and, finding the stale 9 after its own launch, "redo" it from
// them and return MBB_OK (round 3's advisor finding).  Other flags stay for the run's own check.
static int sampler_check_pending(mbb_ctx *c, mbb_sampler_state *s)
{
    if (s->unchecked) {
        int err = 0;
        HIPCHK(hipMemcpyAsync(&err, s->d_err.d(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        s->unchecked = false;
        if (err == 9) {
            HIPCHK(hipMemset(s->d_err.d(), 0, sizeof(int)));
            s->lost = true;
            s->spec_form = 0;
        }
    }
    if (s->lost)
        return fail(MBB_ERR_STATE, "the one-launch sampler run timed out waiting for a half-step; the ensemble it "
                                   "left behind is not a state of the chain: set the sampler's state again");
    return MBB_OK;
}

// How a run is cut into shards.  One shard = the whole half-ensemble (one GPU).
// With an RCCL communicator of G ranks the moving half is cut into G contiguous
// blocks; rank r moves block r and the blocks are exchanged by an in-place
// all-gather of the state rows, so every rank holds the whole, identical ensemble
// before the next half-step.  Option "virtual_ranks" runs the G
// shards one after another on this GPU without any collective -- the same result
// by construction, used to test the sharded launch arithmetic on one device.
struct ShardPlan { int shards, first, last, per; bool collective, xchg; };

static int shard_plan(const mbb_ctx *c, const mbb_sampler_state *s, ShardPlan &p)
{
    const int half = s->nw / 2;
    const bool xchg = c->x.connected && !s->pos6_own.p && c->x.n > 1;
    p.collective = xchg || (c->comm != nullptr && c->nranks > 1);
    const int granks = xchg ? c->x.n : c->nranks, grank = xchg ? c->x.rank : c->rank;
    p.shards = p.collective ? granks : (int)(c->opt.vranks > 1 ? c->opt.vranks : 1);
    if (p.shards > 1 && s->nsrc > 1)
        return fail(MBB_ERR_ARG, "a sharded sampler run needs a single source");
    if (half % p.shards != 0)
        return fail(MBB_ERR_ARG, "nwalkers/2 must be a multiple of the number of ranks");
    p.per = half / p.shards;
    p.first = p.collective ? grank : 0;
    p.last = p.collective ? grank : p.shards - 1;
    p.xchg = xchg;
    return MBB_OK;
}

static int allgather_bytes(mbb_ctx *c, void *base, size_t bytes_per_rank)
{
    // in place: rank r's block already sits at base + r * bytes_per_rank
    int r = g_rccl.AllGather((const char *)base + (size_t)c->rank * bytes_per_rank, base,
                             bytes_per_rank, 0 /* ncclInt8 */, c->comm, c->stream);
    if (r != 0) return fail(MBB_ERR_RCCL, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "ncclAllGather failed");
    return MBB_OK;
}

// How a sampler run goes, decided here alone and once per run: its shards, the walkers of a launch and the form -- the
// first of these whose conditions hold ("Which form a run takes", has what each costs):
//   6  a sharded ensemble with the one-hop exchange, ONE launch per 4096 steps on every rank (k_lnlike SMODE 6): options
//      "lookahead_sampler", "flow_sampler" and "sharded_flow_sampler" on, one source, a step at least, one walker per
//      workgroup, the movers and the workgroups that work ahead of them all resident, the rows in the exchange buffer;
//   7  k_flowm, ONE launch per 4096 steps, every workgroup resident (as form 9; both need "lookahead_sampler" and
//      "flow_sampler" on, one shard, no collective, one source, "flow_min_steps" steps): "merged_flow_sampler" on,
//      "resident_sampler" not 2, up to two walkers per CU, one walker per workgroup;
//   9  k_flowa: "resident_sampler" not 0, and res_w walkers of each half per workgroup fit;
//   2, 1  the launch train, one k_lnlike launch per half-step and shard, with and without the exchange.
// Forms 7 and 9 rest for kFlowRest runs after kFlowStrikes give-ups in a row: such a run takes the train (`resting`,
// counted down by sampler_enqueue).  one_launch_ok false rules out 6, 7 and 9 as option "flow_sampler" 0 does: the redo
// of a run that gave up (sampler_run).
struct RunPlan {
    ShardPlan p;
    int nl = 0;                          // walkers per launch
    int form = 1;                        // 1, 2, 6, 7 or 9, as last_kernel_form reports it
    bool resting = false;                // form 7 or 9 held back by give-ups in a row: one of the runs flow_rest counts
    int res_w = 1;                       // form 9: walkers per workgroup and half
    int rows = 0, aw = 0, n_ahead = 0;   // form 6: the workgroups that work ahead (lookahead_plan)
};

static int plan_sampler_run(const mbb_ctx *c, const mbb_sampler_state *s, int nsteps, bool one_launch_ok, RunPlan &rp)
{
    int rc = shard_plan(c, s, rp.p);
    if (rc) return rc;
    const ShardPlan &p = rp.p;
    const int nl = rp.nl = s->nsrc * p.per;
    int wpb, threads;
    pick_geometry(c, nl, wpb, threads);
    lookahead_plan(c, nl, threads, p.per, rp.rows, rp.aw, rp.n_ahead);
    const bool flow = one_launch_ok && c->opt.lookahead && c->opt.flow && s->nsrc == 1;
    if (flow && p.xchg && c->opt.xflow && nsteps > 0 && wpb == 1 && rp.n_ahead + nl <= c->cu_count &&
        (size_t)s->rows() <= c->x.cap_rows) {
        rp.form = 6;
        return MBB_OK;
    }
    const bool resident = flow && p.shards == 1 && !p.collective && nsteps >= (int)std::max<long>(1, c->opt.flow_min_steps);
    rp.res_w = c->opt.flowr_walkers > 0 ? (int)std::min<long>(c->opt.flowr_walkers, kFaMaxW) : (nl + c->cu_count - 1) / c->cu_count;
    const bool res_fits = rp.res_w >= 1 && rp.res_w <= kFaMaxW && (nl + rp.res_w - 1) / rp.res_w <= c->cu_count;
    if (resident && c->opt.flowm && c->opt.flowr != 2 && 2 * nl <= c->cu_count && wpb == 1) rp.form = 7;
    else if (resident && c->opt.flowr != 0 && res_fits) rp.form = 9;
    else rp.form = p.xchg ? 2 : 1;
    rp.resting = rp.form >= 7 && c->flow_rest > 0;
    if (rp.resting) rp.form = 1;           // (forms 7 and 9 have no exchange)
    return MBB_OK;
}

// What changes from one launch of a sampler run to the next (the form and its shape: RunPlan)
struct SamplerLaunch {
    double *pos6, *chain6;
    unsigned int *nacc;
    int *errflag;
    int s_begin, c_begin, c_count, m_count, nw, step, half, nw_src;
    double stretch_a, zpow;
    unsigned long long seed;
    int persist = 0, parity = 0;         // forms 6, 7, 9: half-steps in this launch; 7, 9: its set of completion counters
    double *spec = nullptr;              // forms 6, 7, 9: the run's device state (form 6: the FlowX)
    unsigned long long serial = 0;       // ... the number of the launch (in its check words and decision words)
};

// The RNG key of step t of a run: it advances over the whole life of the sampler, the chain index restarts
static unsigned long long step_key(const mbb_sampler_state *s, int t)
{
    return s->seed + 0x9E3779B97F4A7C15ull * (s->steps_done + (unsigned long long)t + 1ull);
}

// One launch of sampler form rp.form.  ev: null, or two events to record right before and right behind it.
static int launch_sampler(mbb_ctx *c, const RunPlan &rp, const SamplerLaunch &sl, hipEvent_t *ev)
{
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    if (c->data_nb != c->nb) return fail(MBB_ERR_STATE, "data not set or band count mismatch");
    const int n = rp.nl, form = rp.form;
    LnlikeShape g;
    LikeArgs a;
    int rc = lnlike_shape(c, n, g, a);
    if (rc) return rc;
    a.pos6 = sl.pos6; a.chain6 = sl.chain6; a.nacc = sl.nacc; a.errflag = sl.errflag;
    a.s_begin = sl.s_begin; a.c_begin = sl.c_begin; a.c_count = sl.c_count; a.m_count = sl.m_count; a.nw = sl.nw;
    a.step = sl.step; a.half = sl.half; a.stretch_a = sl.stretch_a; a.zpow = sl.zpow; a.seed = sl.seed; a.nw_src = sl.nw_src;
    a.persist = sl.persist; a.spec = sl.spec; a.flow_serial = sl.serial;   // (forms 1, 2: serial 0, the null `pars`)
    const int spin = (int)((c->opt.flow_spin_log2 & 0x3f) << 24);
    if (form == 7 || form == 9) {
        // the resident sampler forms, every workgroup resident (plan_sampler_run), each with its own LDS plan:
        //   form 7 (k_flowm): 2 n workgroups of (quadrature waves + 5), one per (walker, candidate)
        //   form 9 (k_flowa): ceil(n / W) workgroups of 16 waves, W walkers of each half apiece
        a.spec_cfg = spin | (sl.parity & 1);
        const bool fa = form == 9;
        const int W = fa ? rp.res_w : 1;   // (round 3 also had two pairs of walkers per k_flowm workgroup: superseded by form 9)
        const int wgs = fa ? (n + W - 1) / W : 2 * n;
        const int thr = fa ? 1024 : (std::min(g.threads / 64, 11) + 5) * 64;
        const size_t dyn_limit = dynamic_lds_limit(c), table_bytes = (size_t)c->nchunk * 64 * 3 * sizeof(double);
        auto lds_of = [&](bool cov) { return fa ? flowa_lds(c->nb, c->npart, cov, W) : flowm_lds(c->nb, c->npart, cov, c->nunit); };
        a.wpb = W;
        a.cov_in_lds = (c->has_cov && lds_of(true) <= std::min<size_t>(64 * 1024, dyn_limit)) ? 1 : 0;
        const size_t sm = lds_of(a.cov_in_lds != 0);
        const bool stg = c->opt.stage != 0 && sm + table_bytes + 16 <= dyn_limit;
        const size_t sm_total = sm + (stg ? table_bytes + 16 : 0);
        if (sm_total > dyn_limit) return fail(MBB_ERR_ARG, "band tables too large for the LDS plan");
        c->last_wpb = W; c->last_threads = thr; c->last_grid = wgs; c->last_smem = (long)sm_total;
        c->last_stage = stg ? 1 : 0; c->last_smode = form; c->last_ahead = 0;
        return launch_packed(c, kernel_slot(fa ? kFlowa : kFlowm, model_of(c), stg ? 1 : 0), wgs, thr, sm_total, a, ev);
    }
    // k_lnlike, SMODE = form: 1 the half-step, 2 the half-step with the one-hop exchange, 6 the one-launch look-ahead run
    // across the ranks of a sharded ensemble (slot 3; its single-GPU twin went in round 4: forms 7 and 9 are faster at every
    // ensemble size).  Form 6 dispatches first the n_ahead workgroups that prepare the next half-step -- one row of 16 lanes
    // per (walker, candidate), `rows` of them per wave, `aw` such waves per workgroup (lookahead_plan) -- then the movers.
    int grid = g.grid;
    if (form == 2) a.xargs = c->x.d_args.d();
    if (form == 6) {
        a.spec_cfg = (rp.rows << 8) | (rp.aw << 16) | spin;
        a.n_ahead = rp.n_ahead;
        c->last_grid = grid += rp.n_ahead;
    }
    c->last_smode = form; c->last_ahead = form == 6 ? rp.n_ahead : 0;
    return launch_packed(c, kernel_slot(kLnlike, model_of(c), (form == 6 ? 3 : form) * 2 + (g.stage ? 1 : 0)), grid, g.threads,
                         g.smem, a, ev);
}

// Forms 6, 7 and 9: one launch per 4096 steps.
// Form 6, a sharded ensemble with the one-hop exchange: every rank moves its share of each half and prepares their
// proposals ahead, decisions / rows / words go into every rank's copy of the run's state (behind the rows in the exchange
// buffer) at system scope, and a row's half-step starts when the rows it depends on are done, on whatever GPU.  Around
// each launch: set up this rank's copy, tell the peers (a mover's first store into a peer's copy waits for that peer's
// word), launch, tell the peers the launch has ended, wait for theirs (no store of theirs is in flight any more), bring
// the rows up to date.  Forms 7 and 9: the launch alone -- it files the rows it finds and stores the last ones back.
static int run_one_launch(mbb_ctx *c, mbb_sampler_state *s, const RunPlan &rp, SamplerLaunch &sl, int nsteps, bool store,
                          hipEvent_t *ev)
{
    const size_t R = (size_t)s->rows(), nl = (size_t)rp.nl;
    const bool sharded = rp.form == 6;
    const int rank = sharded ? c->x.rank : 0;
    double *const mine = sharded ? c->x.flow(rank) : nullptr;   // form 6: this rank's copy of the run's state
    sl.spec = sharded ? reinterpret_cast<double *>(c->x.d_flowx.d()) : s->d_spec.d();
    for (int t0 = 0; t0 < nsteps; t0 += 4096) {
        const int nt = std::min(4096, nsteps - t0);
        FlowX fxh;
        if (sharded) {
            memset(&fxh, 0, sizeof fxh);
            for (int r = 0; r < c->x.n; ++r) fxh.base[r] = c->x.flow(r);
            fxh.n = c->x.n; fxh.rank = rank; fxh.run = ++c->x.flow_run;
            HIPCHK(hipMemcpyAsync(c->x.d_flowx.d(), &fxh, sizeof fxh, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_flow_init, dim3((unsigned)((R * 8 + 255) / 256)), dim3(256), 0, c->stream,
                               s->d_pos6, mine, (int)R);
            hipLaunchKernelGGL(k_flow_post, dim3(1), dim3(64), 0, c->stream, c->x.d_flowx.d(), (int)R, 0, fxh.run,
                               (const int *)nullptr);
            HIPCHK(hipGetLastError());
        } else {
            sl.parity = s->flowm_parity;
            s->flowm_parity ^= 1;
        }
        sl.serial = ++g_flow_serial;
        sl.s_begin = rank * rp.p.per; sl.c_begin = s->nw / 2; sl.step = t0; sl.half = 0;
        sl.persist = 2 * nt;
        sl.chain6 = store ? s->d_chain6.d() + (((size_t)rank * nsteps + t0) * 2 * nl) * 6 : nullptr;
        sl.nacc = s->d_nacc.d() + (size_t)rank * 2 * nl;
        sl.seed = step_key(s, t0);
        int rc = launch_sampler(c, rp, sl, ev);
        if (rc) return rc;
        if (sharded) {
            hipLaunchKernelGGL(k_flow_post, dim3(1), dim3(64), 0, c->stream, c->x.d_flowx.d(), (int)R, 1, fxh.run,
                               (const int *)s->d_err.d());
            hipLaunchKernelGGL(k_flow_wait_end, dim3(1), dim3(64), 0, c->stream, flow_view(mine, (int)R).endf, c->x.n, rank,
                               fxh.run, (long long)c->opt.xchg_spin_max, s->d_err.d());
            hipLaunchKernelGGL(k_flow_finish, dim3((unsigned)((R * 6 + 255) / 256)), dim3(256), 0, c->stream,
                               s->d_pos6, mine, (int)R, 2 * nt);
            HIPCHK(hipGetLastError());
        }
    }
    return MBB_OK;
}

// Forms 1 and 2: the launch train, one launch per half-step and shard
static int run_train(mbb_ctx *c, mbb_sampler_state *s, const RunPlan &rp, SamplerLaunch &sl, int nsteps, bool store)
{
    const ShardPlan &p = rp.p;
    const size_t nl = (size_t)rp.nl;
    const int half = s->nw / 2;
    int rc;
    for (int t = 0; t < nsteps; ++t)
        for (int h = 0; h < 2; ++h) {
            const int hb = h ? half : 0;
            for (int r = p.first; r <= p.last; ++r) {
                sl.s_begin = hb + r * p.per; sl.c_begin = h ? 0 : half;
                sl.step = t; sl.half = h;
                sl.chain6 = store ? s->d_chain6.d() + ((((size_t)r * nsteps + t) * 2 + h) * nl) * 6 : nullptr;
                sl.nacc = s->d_nacc.d() + ((size_t)r * 2 + h) * nl;
                sl.seed = step_key(s, t);
                if (p.xchg) ++c->x.seq;
                if ((rc = launch_sampler(c, rp, sl, nullptr))) return rc;
            }
            if (p.collective && !p.xchg &&
                (rc = allgather_bytes(c, s->d_pos6 + (size_t)hb * 6, (size_t)p.per * 6 * sizeof(double))))
                return rc;
        }
    if (p.xchg) {
        // the stream is done only when every peer's last launch has landed here too; chain
        // and acceptance counts stay per rank (the caller gathers them if it wants them)
        if (c->x.seq)
            hipLaunchKernelGGL(k_xchg_wait, dim3(1), dim3(64), 0, c->stream, c->x.flags(c->x.rank), c->x.n,
                               c->x.rank, c->x.seq, (long long)c->opt.xchg_spin_max, s->d_err.d());
        HIPCHK(hipGetLastError());
    } else if (p.collective) {   // every rank ends up with the whole chain and all counts
        if (store && (rc = allgather_bytes(c, s->d_chain6.d(), (size_t)nsteps * 2 * nl * 6 * sizeof(double)))) return rc;
        if ((rc = allgather_bytes(c, s->d_nacc.d(), 2 * nl * sizeof(unsigned int)))) return rc;
    }
    return MBB_OK;
}

// Put the run rp plans on the stream.  backup: forms 7 and 9 keep what the run starts from, so that a run that times out
// (a workgroup that is not resident: another process on the GPU) can be redone as a launch train (sampler_run).  tev: two
// events for mbb_sampler_advance_timed, recorded right before the run's first stream work and right behind its last --
// by the launch itself when the run is one launch of form 7 or 9.
static int sampler_enqueue(mbb_ctx *c, mbb_sampler_state *s, const RunPlan &rp, int nsteps, double stretch_a, bool store,
                           bool backup, hipEvent_t *tev)
{
    s->backup_kept = false;
    if (rp.resting) --c->flow_rest;
    if (rp.form >= 7) {
        const size_t R = (size_t)s->rows();
        if (!s->d_spec.p) {
            // zeroed: the records of a one-launch run are taken by their check words, and freshly
            // allocated memory may hold those of another sampler's run
            if (const int rc = s->d_spec.remake(spec_words(R) * sizeof(double))) return rc;
            HIPCHK(hipMemsetAsync(s->d_spec.d(), 0, spec_words(R) * sizeof(double), c->stream));
        }
        if (backup) {
            if (!s->d_bak.p)
                if (const int rc = s->d_bak.remake(R * 6 * sizeof(double) + R * sizeof(unsigned int))) return rc;
            HIPCHK(hipMemcpyAsync(s->d_bak.d(), s->d_pos6, R * 6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(s->d_bak.d() + R * 6, s->d_nacc.d(), R * sizeof(unsigned int), hipMemcpyDeviceToDevice, c->stream));
        }
        s->backup_kept = backup;
        if (s->spec_form != 7 && s->spec_form != 9) {
            // forms 7 and 9 find their completion counters cleared by the launch before it (either's); after
            // another form (or a run that gave up) has used the memory, once from here
            const FlowMView fvh = flowm_view(s->d_spec.d(), (int)R);
            HIPCHK(hipMemsetAsync(fvh.done, 0, kFmDoneWords * sizeof(unsigned long long), c->stream));
            s->flowm_parity = 0;
        }
        s->spec_form = rp.form;
    }
    const bool carried = tev && rp.form >= 7 && nsteps <= 4096;
    if (tev && !carried) HIPCHK(hipEventRecord(tev[0], c->stream));
    if (rp.p.xchg) {
        // the kernel's view of the exchange for this run, in stream order before its launches
        // (pageable source: staged by the runtime before the call returns)
        XchgArgs xa;
        memset(&xa, 0, sizeof xa);
        for (int r = 0; r < c->x.n; ++r) { xa.xpos[r] = c->x.pos6(r); xa.xflag[r] = c->x.flags(r); }
        xa.xcount = c->x.count(); xa.xn = c->x.n; xa.xrank = c->x.rank;
        xa.xseq0 = c->x.seq; xa.xspin_max = c->opt.xchg_spin_max;
        HIPCHK(hipMemcpyAsync(c->x.d_args.d(), &xa, sizeof xa, hipMemcpyHostToDevice, c->stream));
    }
    SamplerLaunch sl;
    sl.pos6 = s->d_pos6; sl.errflag = s->d_err.d(); sl.nw = s->rows(); sl.nw_src = s->nw;
    sl.stretch_a = stretch_a; sl.zpow = s->zpow; sl.c_count = s->nw / 2; sl.m_count = rp.p.per;
    const int rc = rp.form >= 6 ? run_one_launch(c, s, rp, sl, nsteps, store, carried ? tev : nullptr)
                                : run_train(c, s, rp, sl, nsteps, store);
    if (rc) return rc;
    if (tev && !carried) HIPCHK(hipEventRecord(tev[1], c->stream));
    s->steps_done += (unsigned long long)nsteps;
    return MBB_OK;
}

// mbb_sampler_run once its arguments are checked (one_launch_ok: plan_sampler_run)
static int summary_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                       const mbb_summary_spec *sp, const mbb_summary_out *o);

// (sspec / sout: mbb_sampler_run_summary -- the chain is kept and re-ordered on the device whether or not the caller
// wants it on the host, and summarised there once the run is known to have gone through)
static int sampler_run(mbb_ctx *c, mbb_sampler_state *s, int nsteps, double stretch_a, double *chain, double *lnprob,
                       double *pos_out, double *lnprob_out, double *naccepted, bool one_launch_ok,
                       const mbb_summary_spec *sspec = nullptr, const mbb_summary_out *sout = nullptr)
{
    RunPlan rp;
    int rc = plan_sampler_run(c, s, nsteps, one_launch_ok, rp);
    if (rc) return rc;
    const ShardPlan &p = rp.p;
    const int R = s->rows(), nw = s->nw, half = nw / 2;
    const size_t nl = (size_t)rp.nl;
    const bool to_host = (chain || lnprob) && nsteps > 0;
    const bool store = (to_host || sspec) && nsteps > 0;
    if ((rc = sampler_check_pending(c, s))) return rc;
    if (store) s->resident_nsteps = 0;
    if (store && (size_t)nsteps * R * 6 > s->chain_cap) {
        // (the exact size: a chain is as long as its run)
        const size_t bytes = (size_t)nsteps * R * 6 * sizeof(double);
        s->chain_cap = 0;
        if ((rc = grow(c, s->d_chain6, bytes)) || (rc = grow(c, s->d_chain_out, bytes))) return rc;
        // (a landing buffer the host refuses to pin -- a limit on locked memory -- is done without: the chain
        // then goes straight into the caller's arrays, slower for big chains, never wrong)
        // (only chains big enough to go through it get one: pinning costs a few hundred microseconds)
        s->h_chain.release();
        s->chain_cap = (size_t)nsteps * R * 6;
        s->h_chain_tried = false;
    }
    if (to_host && !s->h_chain.p && !s->h_chain_tried && s->chain_cap * sizeof(double) > kChainDirectBytes) {
        // (a run that only summarises its chain brings none back and pins nothing)
        s->h_chain_tried = true;
        if (s->h_chain.remake(s->chain_cap * sizeof(double))) (void)hipGetLastError();
    }
    if ((rc = sampler_enqueue(c, s, rp, nsteps, stretch_a, store, true, nullptr))) return rc;
    std::vector<double> rows((size_t)R * 6);
    std::vector<unsigned int> nacc(R);
    int err = 0;
    HIPCHK(hipMemcpyAsync(rows.data(), s->d_pos6, rows.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(nacc.data(), s->d_nacc.d(), nacc.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&err, s->d_err.d(), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    // The chain comes back in the caller's layout: re-ordered on the device, copied straight into the
    // caller's arrays.  (A rank of a run sharded with the one-hop exchange holds its own walkers' part
    // only: there the old way, through a staging vector, fills just those rows.)
    const bool direct = store && !p.xchg;
    bool via_pinned = false;
    std::vector<double> ch;
    if (direct) {
        const long long cells = (long long)R * nsteps;
        hipLaunchKernelGGL(k_chain_reorder, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream,
                           (const double *)s->d_chain6.d(), s->d_chain_out.d(), nsteps, nw, half, p.per, s->nsrc, p.shards);
        HIPCHK(hipGetLastError());
        // small chains go straight into the caller's arrays (the runtime stages them through its own pinned
        // buffers); big ones land in ours first -- a D2H into megabytes of pageable, untouched memory runs at
        // ~1 GB/s (measured: 3 MB direct 0.43 ms against 1.35 ms staged; 24 MB direct 25 ms against 6 ms staged)
        via_pinned = to_host && s->h_chain.p != nullptr && (size_t)cells * 6 * sizeof(double) > kChainDirectBytes;
        if (via_pinned) {
            HIPCHK(hipMemcpyAsync(s->h_chain.h(), s->d_chain_out.d(), (size_t)cells * 6 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        } else {
            if (chain) HIPCHK(hipMemcpyAsync(chain, s->d_chain_out.d(), (size_t)cells * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            if (lnprob) HIPCHK(hipMemcpyAsync(lnprob, s->d_chain_out.d() + (size_t)cells * 5, (size_t)cells * sizeof(double),
                                              hipMemcpyDeviceToHost, c->stream));
        }
    } else if (store) {
        ch.resize((size_t)nsteps * R * 6);
        HIPCHK(hipMemcpyAsync(ch.data(), s->d_chain6.d(), ch.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (err) {
        HIPCHK(hipMemset(s->d_err.d(), 0, sizeof(int)));
        if (err == 8) return fail(MBB_ERR_RCCL, "the exchange timed out: a peer did not post its launch");
        if (err == 9 && s->backup_kept) {
            // The one-launch run gave up waiting (not every workgroup was resident): back to the state it
            // started from and the same steps as a train of launches -- the same chain.  The next run takes
            // the one-launch form again; kFlowStrikes give-ups in a row rest it for kFlowRest runs.
            HIPCHK(hipMemcpyAsync(s->d_pos6, s->d_bak.d(), (size_t)R * 6 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(s->d_nacc.d(), s->d_bak.d() + (size_t)R * 6, (size_t)R * sizeof(unsigned int), hipMemcpyDeviceToDevice,
                                  c->stream));
            s->steps_done -= (unsigned long long)nsteps;
            s->spec_form = 0;
            ++c->flow_fallbacks;
            if (++c->flow_strikes >= kFlowStrikes) { c->flow_strikes = 0; c->flow_rest = kFlowRest; }
            return sampler_run(c, s, nsteps, stretch_a, chain, lnprob, pos_out, lnprob_out, naccepted, false, sspec, sout);
        }
        if (err == 9) {
            // (a sharded run: nothing was kept to redo it from)
            s->spec_form = 0;
            s->lost = true;
            return fail(MBB_ERR_STATE, "the one-launch sampler run timed out waiting for a half-step; the ensemble it "
                                       "left behind is not a state of the chain: set the sampler's state again");
        }
        g_err = "lnprob returned NaN or the SED constructor rejected a proposal (row status " +
                std::to_string(err) + ")";
        return MBB_ERR_ARG;
    }
    if (s->backup_kept) c->flow_strikes = 0;                // a one-launch run that went through
    if (direct && via_pinned) {
        const size_t cells = (size_t)R * nsteps;
        if (chain) memcpy(chain, s->h_chain.h(), cells * 5 * sizeof(double));
        if (lnprob) memcpy(lnprob, s->h_chain.h() + cells * 5, cells * sizeof(double));
    }
    for (int i = 0; i < R; ++i) {
        if (pos_out) for (int k = 0; k < 5; ++k) pos_out[(size_t)i * 5 + k] = rows[(size_t)i * 6 + k];
        if (lnprob_out) lnprob_out[i] = rows[(size_t)i * 6 + 5];
    }
    // launch-local order -> rows: shard r, half h, launch index w = src * per + loc
    // (one-hop exchange: only this rank's shard is here; the other rows are left untouched)
    for (int r = p.xchg ? p.first : 0; r <= (p.xchg ? p.last : p.shards - 1); ++r)
        for (int h = 0; h < 2; ++h)
            for (size_t w = 0; w < nl; ++w) {
                const int src = (int)(w / p.per), loc = (int)(w - (size_t)src * p.per);
                const int row = src * nw + (h ? half : 0) + r * p.per + loc;
                if (naccepted) naccepted[row] = (double)nacc[((size_t)r * 2 + h) * nl + w];
                if (!store || direct) continue;
                for (int t = 0; t < nsteps; ++t) {
                    const double *q = &ch[((((size_t)r * nsteps + t) * 2 + h) * nl + w) * 6];
                    if (chain) for (int k = 0; k < 5; ++k) chain[((size_t)row * nsteps + t) * 5 + k] = q[k];
                    if (lnprob) lnprob[(size_t)row * nsteps + t] = q[5];
                }
            }
    if (direct) s->resident_nsteps = nsteps;
    if (sspec) {
        const size_t cells = (size_t)R * nsteps;
        return summary_run(c, s->d_chain_out.d(), s->d_chain_out.d() + cells * 5, s->nsrc, nw, nsteps, sspec, sout);
    }
    return MBB_OK;
}

// Advance nsteps stretch-move steps entirely on the device: 2 nsteps dependent
// launches on the context's stream, no host round trip in between.
// chain [nsrc*nw][nsteps][5] and lnprob [nsrc*nw][nsteps] (emcee's layout per
// source, results.py:154-155) may be NULL; pos_out [nsrc*nw*5], lnprob_out,
// naccepted [nsrc*nw] (running totals).
extern "C" int mbb_sampler_run(mbb_ctx *c, void *sp, int nsteps, double stretch_a, double *chain,
                               double *lnprob, double *pos_out, double *lnprob_out,
                               double *naccepted)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s || nsteps < 0 || !(stretch_a > 1.0)) return fail(MBB_ERR_ARG, "bad sampler arguments");
    if (s->nsrc != c->nsrc) return fail(MBB_ERR_STATE, "number of sources changed since the sampler was made");
    return sampler_run(c, s, nsteps, stretch_a, chain, lnprob, pos_out, lnprob_out, naccepted, true);
}

// Measurement helper: enqueue nsteps steps without storing a chain and without
// synchronising (HIP events around the call time the dependent launch train).
extern "C" int mbb_sampler_advance_async(mbb_ctx *c, void *sp, int nsteps, double stretch_a)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s || nsteps < 0) return fail(MBB_ERR_ARG, "bad sampler arguments");
    if (s->lost) return sampler_check_pending(c, s);
    s->unchecked = true;
    RunPlan rp;
    if ((rc = plan_sampler_run(c, s, nsteps, true, rp))) return rc;
    return sampler_enqueue(c, s, rp, nsteps, stretch_a, false, false, nullptr);
}

// Measurement helper: the same enqueue between the host clock and two events, in one call -- the harness
// around a short timed region is then a few hundred nanoseconds instead of four Python-to-C round trips.
// (The events ride on the launch itself when the run is one: sampler_enqueue.)
extern "C" int mbb_sampler_advance_timed(mbb_ctx *c, void *sp, int nsteps, double stretch_a, double *wall_s,
                                         float *stream_ms)
{
    int rc = use(c);
    if (rc) return rc;
    mbb_sampler_state *s = (mbb_sampler_state *)sp;
    if (!s || nsteps < 0 || !wall_s || !stream_ms) return fail(MBB_ERR_ARG, "bad sampler arguments");
    if (s->lost) return sampler_check_pending(c, s);
    s->unchecked = true;
    if ((rc = c->ev_timed.create())) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    RunPlan rp;
    if ((rc = plan_sampler_run(c, s, nsteps, true, rp))) return rc;
    if ((rc = sampler_enqueue(c, s, rp, nsteps, stretch_a, false, false, c->ev_timed.e))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    const auto t1 = std::chrono::steady_clock::now();
    *wall_s = std::chrono::duration<double>(t1 - t0).count();
    HIPCHK(hipEventElapsedTime(stream_ms, c->ev_timed.e[0], c->ev_timed.e[1]));
    return MBB_OK;
}

// ---- SED-level entry points -------------------------------------------------
static int ensure_sed(mbb_ctx *c, size_t n, size_t nout)
{
    mbb_ctx::SedWork &w = c->sed;
    int rc;
    if (n > w.cap) {
        size_t cap = w.cap ? w.cap : 64;
        while (cap < n) cap *= 2;
        w.cap = 0;
        if ((rc = grow(c, w.pars, cap * 5 * sizeof(double))) || (rc = grow(c, w.status, cap * sizeof(int32_t))) ||
            (rc = grow(c, w.wk, cap * sizeof(WalkerK))))
            return rc;
        w.cap = cap;
    }
    if (nout > w.out_cap) {
        size_t cap = w.out_cap ? w.out_cap : 1024;
        while (cap < nout) cap *= 2;
        w.out_cap = 0;
        if ((rc = grow(c, w.out, cap * sizeof(double)))) return rc;
        w.out_cap = cap;
    }
    return MBB_OK;
}

template <typename F>
static void dispatch_variant(int opthin, int noalpha, F &&f)
{
    if (opthin) { if (noalpha) f(std::true_type(), std::true_type()); else f(std::true_type(), std::false_type()); }
    else { if (noalpha) f(std::false_type(), std::true_type()); else f(std::false_type(), std::false_type()); }
}

// k_prologue on n parameter rows that are on the device already (the rows of a resident chain, or d_sed_pars)
static int launch_prologue(mbb_ctx *c, const double *d_pars, int n, int opthin, int noalpha,
                           double wavenorm, int want_peak, double *d_out6)
{
    const int threads = 64, grid = (n + threads - 1) / threads;
    dispatch_variant(opthin, noalpha, [&](auto OT, auto NA) {
        hipLaunchKernelGGL((k_prologue<decltype(OT)::value, decltype(NA)::value>), dim3(grid),
                           dim3(threads), 0, c->stream, d_pars, n, kUmToGHz / wavenorm,
                           log(kUmToGHz / wavenorm), want_peak, d_out6, c->sed.status.d(),
                           c->sed.wk.d());
    });
    HIPCHK(hipGetLastError());
    return MBB_OK;
}

static int run_prologue(mbb_ctx *c, const double *pars, int n, int opthin, int noalpha,
                        double wavenorm, int want_peak, double *d_out6)
{
    HIPCHK(hipMemcpyAsync(c->sed.pars.d(), pars, (size_t)n * 5 * sizeof(double),
                          hipMemcpyHostToDevice, c->stream));
    return launch_prologue(c, c->sed.pars.d(), n, opthin, noalpha, wavenorm, want_peak, d_out6);
}

extern "C" int mbb_sed_prologue_batch(mbb_ctx *c, const double *pars, int n, int opthin,
                                      int noalpha, double wavenorm, int want_peak, double *out,
                                      int32_t *status)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || !pars || !out) return fail(MBB_ERR_ARG, "bad arguments");
    if ((rc = ensure_sed(c, (size_t)n, (size_t)n * 6))) return rc;
    if ((rc = run_prologue(c, pars, n, opthin, noalpha, wavenorm, want_peak, c->sed.out.d()))) return rc;
    HIPCHK(hipMemcpyAsync(out, c->sed.out.d(), (size_t)n * 6 * sizeof(double),
                          hipMemcpyDeviceToHost, c->stream));
    if (status)
        HIPCHK(hipMemcpyAsync(status, c->sed.status.d(), (size_t)n * sizeof(int32_t),
                              hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

extern "C" int mbb_sed_eval_batch(mbb_ctx *c, const double *pars, int n, int opthin, int noalpha,
                                  double wavenorm, const double *freq, int m, double *out,
                                  int32_t *status)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || m <= 0 || !pars || !freq || !out) return fail(MBB_ERR_ARG, "bad arguments");
    if (n > 65535) return fail(MBB_ERR_ARG, "at most 65535 rows per call");
    const size_t nout = (size_t)n * m;
    if ((rc = ensure_sed(c, (size_t)n, nout + (size_t)m))) return rc;
    double *d_freq = c->sed.out.d() + nout;
    if ((rc = run_prologue(c, pars, n, opthin, noalpha, wavenorm, 0, nullptr))) return rc;
    HIPCHK(hipMemcpyAsync(d_freq, freq, (size_t)m * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int threads = 256;
    dim3 grid((m + threads - 1) / threads, n);
    dispatch_variant(opthin, noalpha, [&](auto OT, auto NA) {
        hipLaunchKernelGGL((k_sed_eval<decltype(OT)::value, decltype(NA)::value>), grid,
                           dim3(threads), 0, c->stream, c->sed.wk.d(), d_freq, m, c->sed.out.d());
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->sed.out.d(), nout * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status)
        HIPCHK(hipMemcpyAsync(status, c->sed.status.d(), (size_t)n * sizeof(int32_t),
                              hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

// Gauss-Legendre nodes and weights on [-1, 1], 64 points (Newton on P_n, Abramowitz & Stegun 25.4.29)
static void gauss_legendre64(double *gx, double *gw)
{
    const int ngl = 64;
    for (int i = 0; i < ngl; ++i) {
        double x = cos(M_PI * (i + 0.75) / (ngl + 0.5)), pp = 1.0;
        for (int it = 0; it < 100; ++it) {
            double p1 = 1.0, p2 = 0.0;
            for (int j = 0; j < ngl; ++j) { double p3 = p2; p2 = p1; p1 = ((2.0 * j + 1.0) * x * p2 - j * p3) / (j + 1.0); }
            pp = ngl * (x * p1 - p2) / (x * x - 1.0);
            const double dx = p1 / pp;
            x -= dx;
            if (fabs(dx) < 1e-16) break;
        }
        gx[i] = x;
        gw[i] = 2.0 / ((1.0 - x * x) * pp * pp);
    }
}

extern "C" int mbb_sed_integrate_batch(mbb_ctx *c, const double *pars, int n, int opthin, int noalpha,
                                       double wavenorm, double numin, double numax, double *out,
                                       int32_t *status)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || !pars || !out || !(numin > 0.0) || !(numax > numin))
        return fail(MBB_ERR_ARG, "bad arguments");
    const int ngl = 64;
    if ((rc = ensure_sed(c, (size_t)n, (size_t)n + 2 * ngl))) return rc;
    double gx[64], gw[64];
    gauss_legendre64(gx, gw);
    double *d_gx = c->sed.out.d() + n, *d_gw = d_gx + ngl;
    if ((rc = run_prologue(c, pars, n, opthin, noalpha, wavenorm, 0, nullptr))) return rc;
    HIPCHK(hipMemcpyAsync(d_gx, gx, sizeof gx, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_gw, gw, sizeof gw, hipMemcpyHostToDevice, c->stream));
    dispatch_variant(opthin, noalpha, [&](auto OT, auto NA) {
        hipLaunchKernelGGL((k_sed_integrate<decltype(OT)::value, decltype(NA)::value>), dim3(n),
                           dim3(64), 0, c->stream, c->sed.wk.d(), numin, numax, d_gx, d_gw, ngl,
                           8, c->sed.out.d());
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->sed.out.d(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status)
        HIPCHK(hipMemcpyAsync(status, c->sed.status.d(), (size_t)n * sizeof(int32_t),
                              hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

// ---- analyses of a resident chain: what the summary, the diagnostics and the marginals share ------------------------
// A work block cut up array by array, by falling alignment: take<T>(n) is its next n values of T.  (A block whose
// arrays go home to the caller is a ResultBlock, mbb_owned.h.)
struct Carve {
    char *p;
    template <typename T> T *take(size_t n) { T *r = (T *)p; p += n * sizeof(T); return r; }
};

// The result list rb of an analysis on the device: its block made big enough, then every array's address handed out.
static int place(mbb_ctx *c, DevBuf &block, ResultBlock &rb) { return rb.place(block, [c] { return sync_stream(c); }); }

// ... and on its way home as one image, behind everything the stream holds: the caller waits, then rb.scatter().
static int fetch_image(mbb_ctx *c, const DevBuf &block, ResultBlock &rb)
{
    HIPCHK(hipMemcpyAsync(rb.image(), block.p, rb.bytes(), hipMemcpyDeviceToHost, c->stream));
    return MBB_OK;
}

// ... for a caller with nothing else to wait for: the image, the wait and the scatter.
static int fetch_home(mbb_ctx *c, const DevBuf &block, ResultBlock &rb)
{
    if (const int rc = fetch_image(c, block, rb)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rb.scatter();
    return MBB_OK;
}

// A launch grid of n blocks, or of a block per `per` of n items, fits in 31 bits.
static int check_grid(size_t n, size_t per = 64) { return n > 0x7fffffffull / per ? fail(MBB_ERR_ARG, "too many sources") : MBB_OK; }

// Whether the context is one rank of several: such a rank holds only its own walkers.
static bool sharded_context(const mbb_ctx *c) { return (c->comm != nullptr && c->nranks > 1) || (c->x.connected && c->x.n > 1); }

// The parameters a fit holds fixed (mbblm::lm_fixed_mask, a device function in this build): the caller's, lambda0 of an
// optically thin model, alpha of a model without one.
static uint32_t fixed_mask(const mbb_ctx *c, const int32_t fixed[5])
{
    uint32_t m = 0;
    for (int i = 0; i < 5; ++i) if (fixed[i]) m |= 1u << i;
    if (c->opthin) m |= 1u << 2;
    if (c->noalpha) m |= 1u << 3;
    return m;
}

// A host chain [cells][5], its lnprob [cells] behind it where given, on the device for as long as run(d_chain) takes.
template <typename F>
static int with_uploaded_chain(mbb_ctx *c, const double *chain, const double *lnprob, size_t cells, F &&run)
{
    Dev<double> buf;
    if (const int rc = buf.remake(cells * (lnprob ? 6 : 5) * sizeof(double))) return rc;
    double *const d = buf.d();
    hipError_t e = hipMemcpyAsync(d, chain, cells * 5 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && lnprob)
        e = hipMemcpyAsync(d + cells * 5, lnprob, cells * sizeof(double), hipMemcpyHostToDevice, c->stream);
    const int rc = e != hipSuccess ? fail(MBB_ERR_HIP, "upload of the chain", e) : run((const double *)d);
    (void)hipStreamSynchronize(c->stream);       // (before buf goes)
    return rc;
}

// The sampler behind a handle whose run can be analysed on this device (verb: what the caller would do to its chain).
static int analysed_sampler(mbb_ctx *c, void *sp, bool args_ok, const char *verb, mbb_sampler_state *&s)
{
    int rc = use(c);
    if (rc) return rc;
    s = (mbb_sampler_state *)sp;
    if (!s || !args_ok) return fail(MBB_ERR_ARG, "bad sampler arguments");
    if (s->nsrc != c->nsrc) return fail(MBB_ERR_STATE, "number of sources changed since the sampler was made");
    ShardPlan p;
    if ((rc = shard_plan(c, s, p))) return rc;
    if (!p.collective) return MBB_OK;
    char buf[160];
    snprintf(buf, sizeof buf, "a sharded sampler run cannot be %s on the device: a rank holds only its own walkers' chain",
             verb);
    return fail(MBB_ERR_STATE, buf);
}

// ... and whether its last stored run is still there in the caller's layout.  (resident_nsteps is made positive by
// sampler_run alone, after k_chain_reorder has written d_chain_out: the chain is never null when it is.)
static int resident_chain(const mbb_sampler_state *s)
{
    if (s->resident_nsteps > 0 && s->d_chain_out.p) return MBB_OK;
    return fail(MBB_ERR_STATE, "no chain of this sampler is resident on the device");
}

// The entry of an analysis of a host chain: check() has the entry's own refusals (a null chain among them where the
// entry hears of it first), then the chain goes up and run(d_chain, d_lnprob or null) works on it.
template <typename Check, typename Run>
static int analyse_chain(mbb_ctx *c, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps, Check &&check,
                         Run &&run)
{
    int rc = use(c);
    if (rc) return rc;
    if ((rc = check())) return rc;                                      // (before the chain is read or uploaded)
    if (!chain) return fail(MBB_ERR_ARG, "bad arguments");
    const size_t cells = (size_t)nsrc * nw * nsteps;
    return with_uploaded_chain(c, chain, lnprob, cells, [&](const double *d) {
        return run(d, lnprob ? d + cells * 5 : nullptr);
    });
}

// ... and of the chain a sampler's last run left on the device: run(d_chain, d_lnprob or null, nsrc, nw, nsteps).
template <typename Run>
static int analyse_sampler(mbb_ctx *c, void *sp, bool args_ok, const char *verb, bool with_lnprob, Run &&run)
{
    mbb_sampler_state *s;
    int rc;
    if ((rc = analysed_sampler(c, sp, args_ok, verb, s)) || (rc = resident_chain(s))) return rc;
    const double *const d = s->d_chain_out.d();
    const size_t cells = (size_t)s->rows() * s->resident_nsteps;
    return run(d, with_lnprob ? d + cells * 5 : nullptr, s->nsrc, s->nw, s->resident_nsteps);
}

// The window [burn::thin] of a chain's nsteps, for every analysis that has one.
static int check_burn_thin(int burn, int thin, int nsteps)
{
    if (burn < 0 || burn >= nsteps || thin < 1) return fail(MBB_ERR_ARG, "bad burn / thin");
    return MBB_OK;
}

// Its kept steps per walker, in 64 bits: nsteps + thin may be beyond an int (at most nsteps once the window is checked).
static long long kept_steps(int burn, int thin, int nsteps)
{
    return ((long long)nsteps - burn + thin - 1) / thin;
}

// The checks of an mbb_summary_spec that every analysis with derived columns makes, in the order they are made.
static int check_window(const mbb_summary_spec *sp, int nsteps)
{
    if (const int rc = check_burn_thin(sp->burn, sp->thin, nsteps)) return rc;
    if (sp->derived & ~7) return fail(MBB_ERR_ARG, "unknown derived column");
    return MBB_OK;
}

// A column's samples are counted in 32 bits (what: the refusal, which differs between the analyses).
static int check_sample_cap(int burn, int thin, int nw, int nsteps, const char *what)
{
    return (long long)nw * kept_steps(burn, thin, nsteps) > 0xffffffffll ? fail(MBB_ERR_ARG, what) : MBB_OK;
}
static int check_sample_cap(const mbb_summary_spec *sp, int nw, int nsteps)
{
    return check_sample_cap(sp->burn, sp->thin, nw, nsteps, "more than 2^32 samples per column");
}

// A checked window of a chain as the kernels read it (the columns and their splits are the caller's).
static void fill_window(mbbc::ChainView &v, const double *d_chain, int nsrc, int nw, int nsteps, int burn, int thin)
{
    v.chain = d_chain;
    v.nsrc = nsrc; v.nw = nw; v.nsteps = nsteps; v.burn = burn; v.thin = thin;
    v.nkept = (int)kept_steps(burn, thin, nsteps);
    v.n = (long long)nw * v.nkept;
}

// ... with every column cut into splits of at most 16384 samples, one split from 256 sources on: the predicted
// fluxes, the goodness of fit and the pointwise terms.  (Not fill_chain_view's rule, which looks at the number of
// active columns: a spec's sums must not depend on how many specs share its group, and the two columns of a goodness
// of fit are cut as the predicted fluxes are.)
static void fill_window_fixed(mbbc::ChainView &v, const double *d_chain, int nsrc, int nw, int nsteps, int burn, int thin)
{
    fill_window(v, d_chain, nsrc, nw, nsteps, burn, thin);
    v.splits = nsrc >= 256 ? 1 : (int)std::min<long long>(mbbc::kMaxSplits, (v.n + 16383) / 16384);
    v.per_split = (v.n + v.splits - 1) / v.splits;
}

// The columns of a checked spec's window of a chain: the active slots, and each column cut into splits of at most
// split_samples samples whose partial results are merged -- unless the (source, column) pairs fill the device by
// themselves: then one workgroup per column.  (With derived columns the splits may differ from a call's without: the
// goodness of fit takes theta-bar from the five parameter columns alone for that reason.)
static void fill_chain_view(mbbc::ChainView &v, const double *d_chain, int nsrc, int nw, int nsteps,
                            const mbb_summary_spec *sp, int split_samples)
{
    fill_window(v, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    v.ncol = 5;
    for (int k = 0; k < 5; ++k) v.col[k] = k;
    for (int k = 0; k < 3; ++k) if ((sp->derived >> k) & 1) v.col[v.ncol++] = 5 + k;
    v.splits = (size_t)nsrc * v.ncol >= 1024
                   ? 1 : (int)std::min<long long>(mbbc::kMaxSplits, (v.n + split_samples - 1) / split_samples);
    v.per_split = (v.n + v.splits - 1) / v.splits;
}

// ---- the derived columns of a chain, for its summary and its marginals ------------------------
constexpr int kSumChunkRows = 1 << 18;      // chain rows a derived column is filled by at a time (bounds the WalkerK buffer)

// What of L_IR and dust mass depends on redshift z and luminosity distance lumdist [Mpc], as postprocess.lir and
// postprocess.dustmass form it: L_IR over observer-frame [wavemin, wavemax] (1 + z) with prefactor 4 pi Mpc^2 / L_sun
// (results.py:661), the dust-mass constants of results.py:775-790.  One place, so that a source of a per-source call
// and the same source summarised alone get the same bits.
static mbbs::SrcConst summary_src_const(const mbb_ctx *c, const mbb_summary_spec *sp, double z, double lumdist)
{
    mbbs::SrcConst e;
    const double opz = 1.0 + z;
    const double minwave = std::min(sp->lir_wavemin, sp->lir_wavemax) * opz,
                 maxwave = std::max(sp->lir_wavemin, sp->lir_wavemax) * opz;
    e.numin = kUmToGHz / maxwave;
    e.numax = kUmToGHz / minwave;
    e.prefac = 3.11749657e4 * (lumdist * lumdist);
    const double dl = lumdist * 3.0856775814913673e24;
    const double wavenorm_rest = c->wavenorm / opz, nunorm_rest = 299792458e6 / wavenorm_rest;
    e.opz = opz;
    e.dl2 = dl * dl;
    e.temp_fac = 6.6260693e-27 * nunorm_rest / 1.38065e-16;
    e.bnu_fac = 2 * 6.6260693e-27 * (nunorm_rest * nunorm_rest * nunorm_rest) / (299792458e2 * 299792458e2);
    e.knu_fac = wavenorm_rest / sp->kappa_wave;
    return e;
}

// The derived columns of spec sp for the resident chain, into a.der[]: the SED kernels are fed the chain's own rows
// (emcee's layout IS an array of 5-parameter rows), a chunk at a time.  The row-status bits met on the way are
// gathered in c->der.colstatus [nsrc][kCols], cleared here first (also when no column is asked for).
static int summary_fill_derived(mbb_ctx *c, const mbb_summary_spec *sp, mbbc::ChainView &a)
{
    using mbbc::kCols;
    int rc, nder = 0;
    mbb_ctx::DerWork &w = c->der;
    const size_t cells = (size_t)a.nsrc * a.nw * a.nsteps;
    const bool per_src = sp->src_redshift && (sp->derived & (MBB_SUM_LIR | MBB_SUM_DUSTMASS));
    const long long per = (long long)a.nw * a.nsteps;      // rows per source
    if ((rc = grow(c, w.colstatus, (size_t)a.nsrc * kCols * sizeof(int)))) return rc;
    int *const colstatus = (int *)w.colstatus.p;
    HIPCHK(hipMemsetAsync(colstatus, 0, (size_t)a.nsrc * kCols * sizeof(int), c->stream));
    for (int k = 0; k < 3; ++k) nder += (sp->derived >> k) & 1;
    if (!nder) return MBB_OK;
    if ((rc = grow(c, w.der, (size_t)nder * cells * sizeof(double)))) return rc;
    double *der[3] = {nullptr, nullptr, nullptr};
    for (int k = 0, i = 0; k < 3; ++k)
        if ((sp->derived >> k) & 1) { der[k] = (double *)w.der.p + (size_t)(i++) * cells; a.der[k] = der[k]; }
    const int ngl = 64;
    const size_t chunk = std::min<size_t>(cells, (size_t)kSumChunkRows);
    if ((rc = ensure_sed(c, chunk, chunk * 6 + 2 * ngl))) return rc;
    double *d_gx = c->sed.out.d() + chunk * 6, *d_gw = d_gx + ngl;
    // what depends on redshift and distance: one entry for the call, or a table with one per source
    mbbs::SrcConst one = {};
    mbbs::SrcConst *d_src = nullptr;
    if (!per_src) {
        if (der[1] || der[2]) one = summary_src_const(c, sp, sp->redshift, sp->lumdist_mpc);
    } else {
        std::vector<mbbs::SrcConst> &h = w.h_src;
        if ((rc = grow(c, w.src, (size_t)a.nsrc * sizeof(mbbs::SrcConst)))) return rc;
        // (h is the pageable source of the upload below: a call that returned early on an error may have left its
        // copy in flight)
        if (w.src_in_flight) HIPCHK(hipStreamSynchronize(c->stream));
        w.src_in_flight = false;
        h.resize((size_t)a.nsrc);
        for (int s = 0; s < a.nsrc; ++s) {
            const double z = sp->src_redshift[s], lumdist = sp->src_lumdist_mpc[s];
            if (z != z || lumdist != lumdist) {             // unknown: every member NaN
                mbbs::SrcConst &e = h[(size_t)s];
                e.numin = e.numax = e.prefac = e.opz = e.dl2 = e.temp_fac = e.bnu_fac = e.knu_fac = NAN;
            } else {
                h[(size_t)s] = summary_src_const(c, sp, z, lumdist);
            }
        }
        d_src = (mbbs::SrcConst *)w.src.p;
        w.src_in_flight = true;
        HIPCHK(hipMemcpyAsync(d_src, h.data(), (size_t)a.nsrc * sizeof(mbbs::SrcConst), hipMemcpyHostToDevice, c->stream));
    }
    if (der[1]) {
        double gx[64], gw[64];
        gauss_legendre64(gx, gw);
        HIPCHK(hipMemcpyAsync(d_gx, gx, sizeof gx, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_gw, gw, sizeof gw, hipMemcpyHostToDevice, c->stream));
    }
    for (size_t off = 0; off < cells; off += chunk) {
        const int n = (int)std::min(chunk, cells - off);
        const double *rows = a.chain + off * 5;
        const int grid = (n + 255) / 256;
        if (der[0]) {
            // peak wavelength: the prologue with want_peak, the fit's model or the reference's (results.py:574-581)
            const int ot = sp->peak_model ? 0 : c->opthin, na = sp->peak_model ? 0 : c->noalpha;
            if ((rc = launch_prologue(c, rows, n, ot, na, c->wavenorm, 1, c->sed.out.d()))) return rc;
            hipLaunchKernelGGL(mbbs::k_sum_take, dim3(grid), dim3(256), 0, c->stream, (const double *)c->sed.out.d(),
                               (const int32_t *)c->sed.status.d(), n, (long long)off, der[0], colstatus,
                               a.nw, a.nsteps, a.burn, a.thin);
            HIPCHK(hipGetLastError());
        }
        if (der[1]) {
            // L_IR as postprocess.lir (summary_src_const)
            if ((rc = launch_prologue(c, rows, n, c->opthin, c->noalpha, c->wavenorm, 0, nullptr))) return rc;
            dispatch_variant(c->opthin, c->noalpha, [&](auto OT, auto NA) {
                if (per_src)
                    hipLaunchKernelGGL((k_sed_integrate_src<decltype(OT)::value, decltype(NA)::value>), dim3(n),
                                       dim3(64), 0, c->stream, c->sed.wk.d(), (const double *)d_src,
                                       (int)(sizeof(mbbs::SrcConst) / sizeof(double)), (long long)off, per, d_gx, d_gw,
                                       ngl, 8, c->sed.out.d());
                else
                    hipLaunchKernelGGL((k_sed_integrate<decltype(OT)::value, decltype(NA)::value>), dim3(n), dim3(64),
                                       0, c->stream, c->sed.wk.d(), one.numin, one.numax, d_gx, d_gw,
                                       ngl, 8, c->sed.out.d());
            });
            HIPCHK(hipGetLastError());
            if (per_src)
                hipLaunchKernelGGL(mbbs::k_sum_lir_src, dim3(grid), dim3(256), 0, c->stream,
                                   (const double *)c->sed.out.d(), (const int32_t *)c->sed.status.d(), n, (long long)off,
                                   (const mbbs::SrcConst *)d_src, der[1], colstatus, a.nw, a.nsteps,
                                   a.burn, a.thin);
            else
                hipLaunchKernelGGL(mbbs::k_sum_lir, dim3(grid), dim3(256), 0, c->stream, (const double *)c->sed.out.d(),
                                   (const int32_t *)c->sed.status.d(), n, (long long)off, one.prefac, der[1],
                                   colstatus, a.nw, a.nsteps, a.burn, a.thin);
            HIPCHK(hipGetLastError());
        }
    }
    if (der[2]) {
        // dust mass: the constants of results.py:775-790 (summary_src_const; k_sum_dustmass_src takes them per source)
        mbbs::DustArgs d;
        d.opz = one.opz;
        d.dl2 = one.dl2;
        d.temp_fac = one.temp_fac;
        d.bnu_fac = one.bnu_fac;
        d.knu_fac = one.knu_fac;
        d.k10 = 10.0 * sp->kappa;
        d.msolar8 = 1.97792e41;
        d.wavenorm = c->wavenorm;
        d.opthin = c->opthin;
        if (per_src)
            hipLaunchKernelGGL(mbbs::k_sum_dustmass_src, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream,
                               a.chain, (long long)cells, per, (const mbbs::SrcConst *)d_src, d, der[2]);
        else
            hipLaunchKernelGGL(mbbs::k_sum_dustmass, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream,
                               a.chain, (long long)cells, d, der[2]);
        HIPCHK(hipGetLastError());
    }
    return MBB_OK;
}

// The redshift and luminosity distance L_IR and dust mass are asked with: one of each for the call, or one per source
// (then NaN is allowed: that source's are unknown).  Nothing is looked at when neither column is asked for.
static int summary_check_cosmology(const mbb_summary_spec *sp, int nsrc)
{
    if (!(sp->derived & (MBB_SUM_LIR | MBB_SUM_DUSTMASS))) return MBB_OK;
    if (!sp->src_redshift != !sp->src_lumdist_mpc)
        return fail(MBB_ERR_ARG, "src_redshift and src_lumdist_mpc go together: both or neither");
    if (!sp->src_redshift) {
        if (!(sp->redshift > -1.0 && sp->redshift < INFINITY && sp->lumdist_mpc > 0.0 && sp->lumdist_mpc < INFINITY))
            return fail(MBB_ERR_ARG, "L_IR and dust mass need a redshift and a luminosity distance");
        return MBB_OK;
    }
    for (int s = 0; s < nsrc; ++s) {
        const double z = sp->src_redshift[s], d = sp->src_lumdist_mpc[s];
        const bool z_ok = z != z || (z > -1.0 && z < INFINITY), d_ok = d != d || (d > 0.0 && d < INFINITY);
        if (z_ok && d_ok) continue;
        char buf[160];
        snprintf(buf, sizeof buf, "source %d: %s %g is neither NaN (unknown) nor %s", s,
                 z_ok ? "luminosity distance" : "redshift", z_ok ? d : z, z_ok ? "finite and > 0" : "finite and > -1");
        return fail(MBB_ERR_ARG, buf);
    }
    return MBB_OK;
}

// ... and everything else the derived columns are computed with.
static int check_derived_settings(const mbb_summary_spec *sp, int nsrc)
{
    int rc;
    if ((rc = summary_check_cosmology(sp, nsrc))) return rc;
    if ((sp->derived & MBB_SUM_LIR) && !(sp->lir_wavemin > 0.0 && sp->lir_wavemax > 0.0))
        return fail(MBB_ERR_ARG, "wavelengths must be positive");
    if ((sp->derived & MBB_SUM_DUSTMASS) && !(sp->kappa > 0.0 && sp->kappa_wave > 0.0))
        return fail(MBB_ERR_ARG, "kappa and kappa_wave must be positive");
    return MBB_OK;
}

// The end of a call that filled derived columns: once the stream is idle, the upload of the per-source constants is over.
static int derived_sync(mbb_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    c->der.src_in_flight = false;
    return MBB_OK;
}

// ---- the column statistics of a chain (mbb_summary.hip.h), for every analysis that reduces columns ------------------
// The percentiles of a call (what: the refusal of a wrong number of them, which names the call) ...
static int check_percentiles(int npct, const double *pct, const char *what)
{
    if (npct < 1 || npct > mbbs::kMaxPct) return fail(MBB_ERR_ARG, what);
    for (int k = 0; k < npct; ++k)
        if (!(pct[k] >= 0.0 && pct[k] <= 100.0)) return fail(MBB_ERR_ARG, "percentiles must be in [0, 100]");
    return MBB_OK;
}

// ... as the kernels read them.
static void set_percentiles(mbbs::SumArgs &a, int npct, const double *pct)
{
    a.npct = npct;
    for (int k = 0; k < npct; ++k) a.pct[k] = pct[k];
}

// The context's work buffers for the statistics of ncolumns columns in splits (part, state), and for their select
// (hist).  An analysis with two views grows for both before it takes a pointer.
static int grow_stats(mbb_ctx *c, size_t ncolumns, int splits)
{
    if (const int rc = grow(c, c->stat.part, ncolumns * splits * mbbs::kStatWords * sizeof(double))) return rc;
    return grow(c, c->stat.state, ncolumns * sizeof(mbbs::ColState));
}
static int grow_select(mbb_ctx *c, size_t ncolumns, int splits)
{
    return grow(c, c->stat.hist, ncolumns * splits * mbbs::kMaxRanks * 256 * sizeof(unsigned int));
}

// The statistics of a's ncolumns columns, and the select's start from them.  (Launches only: the caller asks
// hipGetLastError with its own.)
static void launch_stats(mbb_ctx *c, const mbbs::SumArgs &a, size_t ncolumns)
{
    const dim3 gcol((unsigned)ncolumns, (unsigned)a.splits);
    hipLaunchKernelGGL(mbbs::k_sum_stats, gcol, dim3(mbbs::kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(mbbs::k_sum_begin, dim3((unsigned)((ncolumns + 63) / 64)), dim3(64), 0, c->stream, a);
}

// ... and the select of their percentiles, a byte of the key per pass.
static void launch_select(mbb_ctx *c, const mbbs::SumArgs &a, size_t ncolumns)
{
    const dim3 gcol((unsigned)ncolumns, (unsigned)a.splits);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(mbbs::k_sum_hist, gcol, dim3(mbbs::kThreads), 0, c->stream, a, pass);
        hipLaunchKernelGGL(mbbs::k_sum_pick, dim3((unsigned)ncolumns), dim3(mbbs::kThreads), 0, c->stream, a);
    }
}

// The chain's rows a chunk at a time: their records by launch_prologue (the fit's model), then fill(off, n) on rows
// [off, off + n).
static size_t chunk_rows(size_t cells) { return std::min<size_t>(cells, (size_t)kSumChunkRows); }
template <typename Fill>
static int for_row_chunks(mbb_ctx *c, const double *d_chain, size_t cells, double wavenorm, Fill &&fill)
{
    const size_t chunk = chunk_rows(cells);
    for (size_t off = 0; off < cells; off += chunk) {
        const int n = (int)std::min(chunk, cells - off);
        if (const int rc = launch_prologue(c, d_chain + off * 5, n, c->opthin, c->noalpha, wavenorm, 0, nullptr)) return rc;
        if (const int rc = fill(off, n)) return rc;
    }
    return MBB_OK;
}

// ---- posterior summaries of a chain (mbb_summary.hip.h) ------------------------
// Summarise a chain that is on the device in emcee's layout.  Synchronous; the results land in the caller's arrays.
static int summary_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                       const mbb_summary_spec *sp, const mbb_summary_out *o)
{
    using namespace mbbs;
    static_assert(kCols == MBB_SUMMARY_COLS && kMaxPct == MBB_SUMMARY_MAX_PCT, "summary sizes");
    static_assert(kStEmpty == MBB_SUM_EMPTY && kStNaN == MBB_SUM_HAS_NAN && kStAbsent == MBB_SUM_ABSENT &&
                  kStRowShift == MBB_SUM_ROW_SHIFT, "summary status bits");
    if (!sp || !o || !o->n_used || !o->mean || !o->min || !o->max || !o->pct || !o->status || !o->cov || !o->best ||
        !o->best_index)
        return fail(MBB_ERR_ARG, "null summary argument");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    int rc;
    if ((rc = check_percentiles(sp->npct, sp->pct, "1 to 8 percentiles per summary"))) return rc;
    if ((rc = check_window(sp, nsteps)) || (rc = check_derived_settings(sp, nsrc)) ||
        (rc = check_sample_cap(sp, nw, nsteps)))
        return rc;
    SumArgs a;
    memset(&a, 0, sizeof a);
    fill_chain_view(a, d_chain, nsrc, nw, nsteps, sp, 16384);            // (splits of 64 samples per thread)
    a.lnprob = d_lnprob;
    set_percentiles(a, sp->npct, sp->pct);
    for (int k = 0; k < kCols; ++k) {
        a.has_lo[k] = sp->has_lo[k] != 0; a.has_hi[k] = sp->has_hi[k] != 0;
        a.lo[k] = sp->lo[k]; a.hi[k] = sp->hi[k];
    }
    const size_t ncolumns = (size_t)nsrc * a.ncol, sc = (size_t)nsrc * kCols, ns = (size_t)nsrc;
    mbb_ctx::SumWork &w = c->sum;
    const size_t np = (size_t)sp->npct;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&a.o_nused, sc, o->n_used);
    rb.add(&a.o_mean, sc, o->mean); rb.add(&a.o_min, sc, o->min); rb.add(&a.o_max, sc, o->max);
    rb.add(&a.o_pct, sc * np, o->pct);
    rb.add(&a.o_cov, ns * 25, o->cov); rb.add(&a.o_best, ns * 6, o->best);
    rb.add(&a.o_status, sc, o->status); rb.add(&a.o_bestidx, ns * 2, o->best_index);
    if ((rc = grow_stats(c, ncolumns, a.splits)) || (rc = grow_select(c, ncolumns, a.splits))) return rc;
    if ((rc = grow(c, w.covpart, ns * a.splits * kCovWords * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.part = (double *)c->stat.part.p; a.state = (ColState *)c->stat.state.p; a.hist = (unsigned int *)c->stat.hist.p;
    a.covpart = (double *)w.covpart.p;
    if ((rc = summary_fill_derived(c, sp, a))) return rc;
    a.colstatus = (int *)c->der.colstatus.p;
    launch_stats(c, a, ncolumns);
    launch_select(c, a, ncolumns);
    hipLaunchKernelGGL(k_sum_cov, dim3((unsigned)nsrc, (unsigned)a.splits), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_sum_finish, dim3((unsigned)(((size_t)nsrc * kCols + 63) / 64)), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    if ((rc = fetch_image(c, w.outbuf, rb)) || (rc = derived_sync(c))) return rc;
    rb.scatter();
    return MBB_OK;
}

extern "C" int mbb_chain_summary(mbb_ctx *c, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                                 const mbb_summary_spec *spec, const mbb_summary_out *out)
{
    // (per-source values are checked before the chain goes up; everything else where it always was, in summary_run)
    return analyse_chain(c, chain, lnprob, nsrc, nw, nsteps, [&]() -> int {
        if (!chain || !lnprob || nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "bad arguments");
        return spec && (spec->src_redshift || spec->src_lumdist_mpc) ? summary_check_cosmology(spec, nsrc) : MBB_OK;
    }, [&](const double *d, const double *dl) { return summary_run(c, d, dl, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_run_summary(mbb_ctx *c, void *sp, int nsteps, double stretch_a, const mbb_summary_spec *spec,
                                       const mbb_summary_out *out, double *chain, double *lnprob, double *pos_out,
                                       double *lnprob_out, double *naccepted)
{
    mbb_sampler_state *s;
    int rc = analysed_sampler(c, sp, nsteps >= 0 && stretch_a > 1.0 && spec && out, "summarised", s);
    if (rc) return rc;
    // (per-source values are checked before the run; everything else where it always was, in summary_run)
    if ((spec->src_redshift || spec->src_lumdist_mpc) && (rc = summary_check_cosmology(spec, s->nsrc))) return rc;
    if (nsteps == 0) {
        if ((rc = resident_chain(s))) return rc;
        const size_t cells = (size_t)s->rows() * s->resident_nsteps;
        return summary_run(c, s->d_chain_out.d(), s->d_chain_out.d() + cells * 5, s->nsrc, s->nw, s->resident_nsteps, spec, out);
    }
    return sampler_run(c, s, nsteps, stretch_a, chain, lnprob, pos_out, lnprob_out, naccepted, true, spec, out);
}

// ---- convergence diagnostics of a chain (mbb_diag.hip.h) ------------------------
// The argument checks of a diagnostics call: before anything is allocated or uploaded.
static int diag_check(int nsrc, int nw, int nsteps, const mbb_diag_spec *sp, const mbb_diag_out *o)
{
    if (!sp || !o || !o->tau || !o->ess || !o->rhat || !o->window || !o->status)
        return fail(MBB_ERR_ARG, "null diagnostics argument");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (sp->burn < 0 || sp->burn >= nsteps) return fail(MBB_ERR_ARG, "burn leaves no step of the chain");
    if (sp->method != MBB_DIAG_MEAN && sp->method != MBB_DIAG_WALKERS)
        return fail(MBB_ERR_ARG, "unknown diagnostics method (0 mean, 1 walkers)");
    if (!(sp->c > 0.0 && sp->c < INFINITY)) return fail(MBB_ERR_ARG, "the window factor c must be positive");
    if (!(sp->tol >= 0.0 && sp->tol < INFINITY)) return fail(MBB_ERR_ARG, "tol must not be negative");
    const int n = nsteps - sp->burn;
    if (n > mbbg::kMaxSteps) return fail(MBB_ERR_ARG, "more than 16384 kept steps per series: raise burn");
    if (sp->nacf < 0 || sp->nacf > n) return fail(MBB_ERR_ARG, "nacf must be between 0 and the number of kept steps");
    return check_grid((size_t)nsrc * 5);
}

// Diagnose a chain that is on the device in emcee's layout.  Synchronous; the results land in the caller's arrays.
static int diag_run(mbb_ctx *c, const double *d_chain, int nsrc, int nw, int nsteps, const mbb_diag_spec *sp,
                    const mbb_diag_out *o)
{
    using namespace mbbg;
    static_assert(kStShort == MBB_DIAG_SHORT && kStConst == MBB_DIAG_CONSTANT && kStNaN == MBB_DIAG_HAS_NAN &&
                  kStUnreliable == MBB_DIAG_UNRELIABLE && kMaxSteps == MBB_DIAG_MAX_STEPS, "diagnostics constants");
    int rc;
    if ((rc = diag_check(nsrc, nw, nsteps, sp, o))) return rc;
    const int n = nsteps - sp->burn;
    const size_t ncol = (size_t)nsrc * 5, nacf = o->acf ? (size_t)sp->nacf : 0;
    DiagArgs a;
    memset(&a, 0, sizeof a);
    a.chain = d_chain;
    a.nsrc = nsrc; a.nw = nw; a.nsteps = nsteps; a.burn = sp->burn; a.n = n;
    a.method = sp->method; a.nacf = (int)nacf; a.c = sp->c; a.tol = sp->tol;
    mbb_ctx::DiagWork &w = c->diag;
    ResultBlock rb;
    rb.add(&a.o_tau, ncol, o->tau); rb.add(&a.o_ess, ncol, o->ess); rb.add(&a.o_rhat, ncol, o->rhat);
    rb.add(&a.o_acf, ncol * nacf, o->acf);                   // (empty, and null to the kernels, when not asked for)
    rb.add(&a.o_window, ncol, o->window); rb.add(&a.o_status, ncol, o->status);
    if (sp->method == MBB_DIAG_MEAN && (rc = grow(c, w.mean, ncol * n * sizeof(double)))) return rc;
    if ((rc = grow(c, w.seq, ncol * nw * 4 * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.mean = (double *)w.mean.p; a.seq = (double *)w.seq.p;
    const size_t lds = acf_lds_bytes(n);
    if (lds > 60 * 1024 && lds > w.lds_granted) {
        // (beyond 64 KB of LDS per workgroup, the kernel's 2.3 KB of static LDS included, its dynamic-LDS ceiling has
        // to be raised: from 60 KB of dynamic on, once per size)
        const size_t want = std::min<size_t>((lds + 16383) & ~(size_t)16383, acf_lds_bytes(kMaxSteps));
        HIPCHK(hipFuncSetAttribute((const void *)k_diag_acf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want));
        w.lds_granted = want;
    }
    if (sp->method == MBB_DIAG_MEAN) {
        const size_t per = ((size_t)n * 5 + kThreads - 1) / kThreads;
        if ((rc = check_grid(per * nsrc, 1))) return rc;
        hipLaunchKernelGGL(k_diag_mean, dim3((unsigned)(per * nsrc)), dim3(kThreads), 0, c->stream, a);
    }
    hipLaunchKernelGGL(k_diag_acf, dim3((unsigned)ncol), dim3(kThreads), lds, c->stream, a);
    // a wave per walker; when the columns do not fill the device by themselves, the walkers are spread over y
    const int waves = kThreads / 64;
    const int gy = ncol >= 1024 ? 1 : std::min(64, (nw + waves - 1) / waves);
    hipLaunchKernelGGL(k_diag_seq, dim3((unsigned)ncol, (unsigned)gy), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_diag_rhat, dim3((unsigned)ncol), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return fetch_home(c, w.outbuf, rb);
}

extern "C" int mbb_chain_diagnostics(mbb_ctx *c, const double *chain, int nsrc, int nw, int nsteps,
                                     const mbb_diag_spec *spec, const mbb_diag_out *out)
{
    return analyse_chain(c, chain, nullptr, nsrc, nw, nsteps, [&] {
        return !chain ? fail(MBB_ERR_ARG, "bad arguments") : diag_check(nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *) { return diag_run(c, d, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_diagnostics(mbb_ctx *c, void *sp, const mbb_diag_spec *spec, const mbb_diag_out *out)
{
    return analyse_sampler(c, sp, spec && out, "diagnosed", false, [&](const double *d, const double *, int nsrc, int nw, int nsteps) {
        return diag_run(c, d, nsrc, nw, nsteps, spec, out);
    });
}

// ---- binned marginals of a chain (mbb_marginals.hip.h) ------------------------
// The argument checks of a marginals call: before anything is allocated or uploaded.
static int marg_check(int nsrc, int nw, int nsteps, const mbb_marginals_spec *sp, const mbb_marginals_out *o)
{
    using namespace mbbm;
    static_assert(kCols == MBB_SUMMARY_COLS && kMaxBins == MBB_MARG_MAX_BINS && kMaxBins2 == MBB_MARG_MAX_BINS2 &&
                  kMaxPairs == MBB_MARG_MAX_PAIRS, "marginals sizes");
    static_assert(kStEmpty == MBB_MARG_EMPTY && kStNonfinite == MBB_MARG_NONFINITE && kStAbsent == MBB_MARG_ABSENT &&
                  kStRowShift == MBB_MARG_ROW_SHIFT && kStRowShift == mbbs::kStRowShift, "marginals status bits");
    if (!sp || !o || !sp->summary) return fail(MBB_ERR_ARG, "null marginals argument");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (sp->nbins < 1 || sp->nbins > kMaxBins) return fail(MBB_ERR_ARG, "nbins must be between 1 and 4096");
    if (sp->nbins2 < 0 || sp->nbins2 > kMaxBins2) return fail(MBB_ERR_ARG, "nbins2 must be between 0 and 100");
    if (sp->npairs < 0 || sp->npairs > kMaxPairs) return fail(MBB_ERR_ARG, "0 to 28 pairs per call");
    if (sp->npairs > 0 && sp->nbins2 == 0) return fail(MBB_ERR_ARG, "pairs need nbins2 > 0");
    const bool two = sp->nbins2 > 0 && sp->npairs > 0;
    if (!o->counts1 || !o->edges1 || !o->n_used || !o->n_below || !o->n_above || !o->n_nonfinite || !o->status ||
        (two && !o->counts2) || (sp->nbins2 > 0 && !o->edges2))
        return fail(MBB_ERR_ARG, "null marginals argument");
    const mbb_summary_spec *ss = sp->summary;
    int rc;
    if ((rc = check_window(ss, nsteps))) return rc;
    const auto present = [&](int slot) { return slot >= 0 && slot < kCols && (slot < 5 || ((ss->derived >> (slot - 5)) & 1)); };
    for (int k = 0; k < sp->npairs; ++k) {
        const int a = sp->pairs[k][0], b = sp->pairs[k][1];
        if (!present(a) || !present(b)) return fail(MBB_ERR_ARG, "a pair names a column that is absent");
        if (a >= b) return fail(MBB_ERR_ARG, "a pair (a, b) needs a < b");
    }
    for (int k = 0; k < kCols; ++k) {
        if (!sp->has_range[k]) continue;
        const double lo = sp->lo[k], hi = sp->hi[k];
        if (!(lo - lo == 0.0 && hi - hi == 0.0 && lo < hi && (hi - lo) - (hi - lo) == 0.0))
            return fail(MBB_ERR_ARG, "a range must be finite with lo < hi");
    }
    if ((rc = check_derived_settings(ss, nsrc)) || (rc = check_sample_cap(ss, nw, nsteps))) return rc;
    return check_grid((size_t)nsrc * (kCols + kMaxPairs));
}

// Bin a chain that is on the device in emcee's layout.  Synchronous; the results land in the caller's arrays.
static int marg_run(mbb_ctx *c, const double *d_chain, int nsrc, int nw, int nsteps, const mbb_marginals_spec *sp,
                    const mbb_marginals_out *o)
{
    using namespace mbbm;
    int rc;
    if ((rc = marg_check(nsrc, nw, nsteps, sp, o))) return rc;
    MargArgs a;
    memset(&a, 0, sizeof a);
    // (summary_run's splits at a finer grain: a table costs no floating-point tree over the splits, and a single
    // source's five columns are otherwise twenty workgroups)
    fill_chain_view(a, d_chain, nsrc, nw, nsteps, sp->summary, kSplitSamples);
    a.nbins = sp->nbins;
    a.nbins2 = sp->nbins2;
    a.npairs = sp->nbins2 > 0 ? sp->npairs : 0;
    for (int k = 0; k < a.npairs; ++k) { a.pair[k][0] = sp->pairs[k][0]; a.pair[k][1] = sp->pairs[k][1]; }
    for (int k = 0; k < kCols; ++k) { a.has_range[k] = sp->has_range[k] != 0; a.lo[k] = sp->lo[k]; a.hi[k] = sp->hi[k]; }
    const size_t ncolumns = (size_t)nsrc * a.ncol, npairs = (size_t)nsrc * a.npairs;
    const size_t sc = (size_t)nsrc * kCols, nb = (size_t)a.nbins, nb2 = (size_t)a.nbins2;
    const size_t n_e1 = sc * (nb + 1), n_e2 = nb2 ? sc * (nb2 + 1) : 0, n_c1 = sc * nb, n_c2 = npairs * nb2 * nb2;
    ResultBlock rb;                              // doubles, 64-bit counts, 32-bit words
    // (edges2 and counts2 are empty, and null to the kernels, without 2-d tables: k_marg_edges writes edges2 only with
    // nbins2 > 0, k_marg_hist2 is not launched and k_marg_merge has no pair block without pairs)
    rb.add(&a.o_edges1, n_e1, o->edges1); rb.add(&a.o_edges2, n_e2, o->edges2);
    rb.add(&a.o_used, sc, o->n_used); rb.add(&a.o_below, sc, o->n_below);
    rb.add(&a.o_above, sc, o->n_above); rb.add(&a.o_nonfinite, sc, o->n_nonfinite);
    rb.add(&a.o_counts1, n_c1, o->counts1); rb.add(&a.o_counts2, n_c2, o->counts2);
    rb.add(&a.o_status, sc, o->status);
    mbb_ctx::MargWork &w = c->marg;
    if ((rc = grow(c, w.extent, ncolumns * a.splits * 2 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.range, sc * sizeof(Range)))) return rc;
    if ((rc = grow(c, w.part1, ncolumns * a.splits * (nb + kTail) * sizeof(unsigned int)))) return rc;
    if (npairs && (rc = grow(c, w.part2, npairs * a.splits * nb2 * nb2 * sizeof(unsigned int)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.extent = (double *)w.extent.p; a.range = (Range *)w.range.p;
    a.part1 = (unsigned int *)w.part1.p; a.part2 = (unsigned int *)w.part2.p;
    if ((rc = summary_fill_derived(c, sp->summary, a))) return rc;
    a.colstatus = (const int *)c->der.colstatus.p;
    const dim3 gcol((unsigned)ncolumns, (unsigned)a.splits);
    hipLaunchKernelGGL(k_marg_extent, gcol, dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_marg_edges, dim3((unsigned)sc), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_marg_hist1, gcol, dim3(kThreads), 0, c->stream, a);
    if (npairs)
        hipLaunchKernelGGL(k_marg_hist2, dim3((unsigned)npairs, (unsigned)a.splits), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_marg_merge, dim3((unsigned)(sc + npairs)), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    // (the tables are large: each array straight into the caller's, no image in between)
    if ((rc = rb.each([&](void *dst, size_t off, size_t bytes) -> int {
            HIPCHK(hipMemcpyAsync(dst, (const char *)w.outbuf.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
            return MBB_OK;
        })))
        return rc;
    return derived_sync(c);
}

extern "C" int mbb_chain_marginals(mbb_ctx *c, const double *chain, int nsrc, int nw, int nsteps,
                                   const mbb_marginals_spec *spec, const mbb_marginals_out *out)
{
    return analyse_chain(c, chain, nullptr, nsrc, nw, nsteps, [&] {
        return !chain ? fail(MBB_ERR_ARG, "bad arguments") : marg_check(nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *) { return marg_run(c, d, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_marginals(mbb_ctx *c, void *sp, const mbb_marginals_spec *spec, const mbb_marginals_out *out)
{
    return analyse_sampler(c, sp, spec && out, "binned", false, [&](const double *d, const double *, int nsrc, int nw, int nsteps) {
        return marg_run(c, d, nsrc, nw, nsteps, spec, out);
    });
}

// ---- predicted fluxes of a chain (mbb_predict.hip.h) ------------------------
// The argument checks of a prediction call: before anything is allocated, uploaded or launched.
static int pred_check(int nsrc, int nw, int nsteps, const mbb_predict_spec *sp, const mbb_predict_out *o)
{
    using namespace mbbp;
    static_assert(kMaxSpecs == MBB_PRED_MAX_SPECS && kMaxSamples == MBB_PRED_MAX_SAMPLES, "prediction sizes");
    if (!sp || !o || !sp->sample_off || !sp->freq || !sp->weight || !o->n_used || !o->mean || !o->min || !o->max ||
        !o->pct || !o->status)
        return fail(MBB_ERR_ARG, "null prediction argument");
    const bool clip = sp->has_lo || sp->has_hi || sp->lo || sp->hi;
    if (clip && !(sp->has_lo && sp->has_hi && sp->lo && sp->hi))
        return fail(MBB_ERR_ARG, "has_lo, has_hi, lo and hi go together: all or none");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (sp->nspec < 1 || sp->nspec > kMaxSpecs) return fail(MBB_ERR_ARG, "1 to 128 specs per prediction call");
    if (sp->sample_off[0] != 0) return fail(MBB_ERR_ARG, "sample_off must start at 0");
    for (int s = 0; s < sp->nspec; ++s) {
        if (sp->sample_off[s + 1] <= sp->sample_off[s]) return fail(MBB_ERR_ARG, "a spec has no samples");
        if (sp->sample_off[s + 1] > kMaxSamples) return fail(MBB_ERR_ARG, "more than 32768 samples in a prediction call");
    }
    const int ns = sp->sample_off[sp->nspec];
    for (int i = 0; i < ns; ++i) {
        if (!(sp->freq[i] > 0.0 && sp->freq[i] < INFINITY)) return fail(MBB_ERR_ARG, "a frequency must be finite and positive");
        if (!(sp->weight[i] - sp->weight[i] == 0.0)) return fail(MBB_ERR_ARG, "a weight must be finite");
    }
    int rc;
    if ((rc = check_percentiles(sp->npct, sp->pct, "1 to 8 percentiles per prediction call"))) return rc;
    if ((rc = check_burn_thin(sp->burn, sp->thin, nsteps))) return rc;
    if (!(sp->wavenorm >= 0.0 && sp->wavenorm < INFINITY)) return fail(MBB_ERR_ARG, "wavenorm must be positive (0: the context's)");
    if ((rc = check_sample_cap(sp->burn, sp->thin, nw, nsteps, "more than 2^32 - 1 samples per column"))) return rc;
    return check_grid((size_t)nsrc * mbbp::kGroup);
}

// Predict from a chain that is on the device in emcee's layout.  Synchronous; the results land in the caller's arrays.
static int pred_run(mbb_ctx *c, const double *d_chain, int nsrc, int nw, int nsteps, const mbb_predict_spec *sp,
                    const mbb_predict_out *o)
{
    using namespace mbbp;
    int rc;
    if ((rc = pred_check(nsrc, nw, nsteps, sp, o))) return rc;
    const int nspec = sp->nspec, ns = sp->sample_off[nspec];
    const size_t cells = (size_t)nsrc * nw * nsteps, sn = (size_t)nsrc * nspec, np = (size_t)sp->npct;
    const double wavenorm = sp->wavenorm > 0.0 ? sp->wavenorm : c->wavenorm;
    mbbs::SumArgs a;
    memset(&a, 0, sizeof a);
    fill_window_fixed(a, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    set_percentiles(a, sp->npct, sp->pct);
    const int ngmax = std::min(nspec, kGroup);
    mbb_ctx::PredWork &w = c->pred;
    FinishArgs f;
    f.nspec = nspec;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&f.o_nused, sn, o->n_used);
    rb.add(&f.o_mean, sn, o->mean); rb.add(&f.o_min, sn, o->min); rb.add(&f.o_max, sn, o->max);
    rb.add(&f.o_pct, sn * np, o->pct);
    rb.add(&f.o_status, sn, o->status);
    if ((rc = grow(c, w.samples, (size_t)ns * 3 * sizeof(double)))) return rc;
    if ((rc = grow_stats(c, (size_t)nsrc * ngmax, a.splits)) || (rc = grow_select(c, (size_t)nsrc * ngmax, a.splits))) return rc;
    if ((rc = grow(c, w.status, sn * sizeof(int)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    if ((rc = grow(c, c->der.der, (size_t)ngmax * cells * sizeof(double)))) return rc;
    if ((rc = ensure_sed(c, chunk_rows(cells), 0))) return rc;
    a.part = (double *)c->stat.part.p; a.state = (mbbs::ColState *)c->stat.state.p; a.hist = (unsigned int *)c->stat.hist.p;
    f.pstatus = (const int *)w.status.p;
    double *const d_nu = (double *)w.samples.p, *const d_ln = d_nu + ns, *const d_wt = d_ln + ns;
    // (the caller's arrays are pageable: the copies below have read them when they return)
    HIPCHK(hipMemcpyAsync(d_nu, sp->freq, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_wt, sp->weight, (size_t)ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pred_lnnu, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, (const double *)d_nu, ns, d_ln);
    HIPCHK(hipMemsetAsync(w.status.p, 0, sn * sizeof(int), c->stream));
    for (int spec0 = 0; spec0 < nspec; spec0 += kGroup) {
        const int ng = std::min(kGroup, nspec - spec0);
        FillArgs fa;
        memset(&fa, 0, sizeof fa);
        fa.wk = c->sed.wk.d(); fa.status = c->sed.status.d();
        fa.nu = d_nu; fa.lnnu = d_ln; fa.wt = d_wt;
        fa.ng = ng; fa.pstatus = (int *)w.status.p; fa.nspec = nspec; fa.spec0 = spec0;
        fa.nw = nw; fa.nsteps = nsteps; fa.burn = sp->burn; fa.thin = sp->thin;
        int staged = 0;
        a.ncol = ng;
        for (int g = 0; g < ng; ++g) {
            const int s = spec0 + g;
            fa.s0[g] = sp->sample_off[s]; fa.s1[g] = sp->sample_off[s + 1];
            fa.single[g] = fa.s1[g] - fa.s0[g] == 1 && sp->weight[fa.s0[g]] == 1.0;
            fa.l0[g] = staged;
            if (!fa.single[g]) staged += fa.s1[g] - fa.s0[g];
            fa.col[g] = (double *)c->der.der.p + (size_t)g * cells;
            a.der[g] = fa.col[g];
            a.col[g] = 5 + g;
            a.has_lo[5 + g] = sp->has_lo ? sp->has_lo[s] != 0 : 0; a.has_hi[5 + g] = sp->has_hi ? sp->has_hi[s] != 0 : 0;
            a.lo[5 + g] = sp->lo ? sp->lo[s] : 0.0; a.hi[5 + g] = sp->hi ? sp->hi[s] : 0.0;
        }
        const bool stage = staged > 0 && staged <= kLdsSamples;
        fa.nstaged = stage ? staged : 0;
        const size_t lds = (size_t)fa.nstaged * 3 * sizeof(double);
        if ((rc = for_row_chunks(c, d_chain, cells, wavenorm, [&](size_t off, int n) -> int {
            fa.n = n; fa.off = (long long)off;
            const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
            dispatch_variant(c->opthin, c->noalpha, [&](auto OT, auto NA) {
                if (stage)
                    hipLaunchKernelGGL((k_pred_fill<decltype(OT)::value, decltype(NA)::value, true>), grid, dim3(kThreads), lds,
                                       c->stream, fa);
                else
                    hipLaunchKernelGGL((k_pred_fill<decltype(OT)::value, decltype(NA)::value, false>), grid, dim3(kThreads), 0,
                                       c->stream, fa);
            });
            HIPCHK(hipGetLastError());
            return MBB_OK;
        })))
            return rc;
        const size_t ncolumns = (size_t)nsrc * ng;
        launch_stats(c, a, ncolumns);
        launch_select(c, a, ncolumns);
        f.spec0 = spec0;
        hipLaunchKernelGGL(k_pred_finish, dim3((unsigned)((ncolumns + 63) / 64)), dim3(64), 0, c->stream, a, f);
        HIPCHK(hipGetLastError());
    }
    return fetch_home(c, w.outbuf, rb);
}

extern "C" int mbb_chain_predict(mbb_ctx *c, const double *chain, int nsrc, int nw, int nsteps,
                                 const mbb_predict_spec *spec, const mbb_predict_out *out)
{
    return analyse_chain(c, chain, nullptr, nsrc, nw, nsteps, [&] {
        return !chain ? fail(MBB_ERR_ARG, "bad arguments") : pred_check(nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *) { return pred_run(c, d, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_predict(mbb_ctx *c, void *sp, const mbb_predict_spec *spec, const mbb_predict_out *out)
{
    return analyse_sampler(c, sp, spec && out, "predicted from", false, [&](const double *d, const double *, int nsrc, int nw, int nsteps) {
        return pred_run(c, d, nsrc, nw, nsteps, spec, out);
    });
}

// ---- posterior draws of a chain (mbb_draws.hip.h) ------------------------
// The checks of the picks themselves: sizes, how, and the window (ss: burn and thin are looked at).
static int draws_check_picks(int nsrc, int nw, int nsteps, const mbb_summary_spec *ss, int n, int how)
{
    static_assert(mbbw::kMaxDraws == MBB_DRAWS_MAX && mbbw::kRandom == MBB_DRAWS_RANDOM && mbbw::kEven == MBB_DRAWS_EVEN,
                  "draws constants");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (n < 1) return fail(MBB_ERR_ARG, "at least one draw per source");
    if (n > mbbw::kMaxDraws) return fail(MBB_ERR_ARG, "more than 2^24 draws per source");
    if ((long long)nsrc * n > 0x7fffffffll) return fail(MBB_ERR_ARG, "more than 2^31 - 1 draws per call");
    if (how != mbbw::kRandom && how != mbbw::kEven) return fail(MBB_ERR_ARG, "unknown how (0 random, 1 even)");
    int rc;
    if ((rc = check_window(ss, nsteps)) || (rc = check_sample_cap(ss, nw, nsteps))) return rc;
    return MBB_OK;
}

// The argument checks of a draws call: before anything is allocated, uploaded or launched.
static int draws_check(int nsrc, int nw, int nsteps, const mbb_draws_spec *sp, const mbb_draws_out *o)
{
    if (!sp || !o || !sp->summary || !o->rows || !o->lnprob || !o->index || !o->status)
        return fail(MBB_ERR_ARG, "null draws argument");
    int rc;
    if ((rc = draws_check_picks(nsrc, nw, nsteps, sp->summary, sp->n, sp->how))) return rc;
    for (int k = 0; k < 3; ++k)
        if (((sp->summary->derived >> k) & 1) && !o->derived[k]) return fail(MBB_ERR_ARG, "null draws argument");
    return check_derived_settings(sp->summary, nsrc);
}

// The picks of a checked call as kernel arguments (the chain may be null: k_draw_index reads none).
static void fill_draw_args(mbbw::DrawArgs &a, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                           const mbb_summary_spec *ss, int n, int how, unsigned long long seed)
{
    memset(&a, 0, sizeof a);
    fill_chain_view(a, d_chain, nsrc, nw, nsteps, ss, 16384);       // (the splits are not used)
    a.lnprob = d_lnprob;
    a.ndraw = n; a.how = how; a.seed = seed;
}

// Draw from a chain that is on the device in emcee's layout (d_lnprob may be null).  Synchronous; the results land in
// the caller's arrays.
static int draws_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                     const mbb_draws_spec *sp, const mbb_draws_out *o)
{
    using namespace mbbw;
    using mbbc::kCols;
    int rc;
    if ((rc = draws_check(nsrc, nw, nsteps, sp, o))) return rc;
    DrawArgs a;
    fill_draw_args(a, d_chain, d_lnprob, nsrc, nw, nsteps, sp->summary, sp->n, sp->how, sp->seed);
    const size_t nd = (size_t)nsrc * sp->n;
    mbb_ctx::DrawWork &w = c->draw;
    if ((rc = grow(c, w.rows, nd * 5 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.aux, nd * (sizeof(double) + 2 * sizeof(int))))) return rc;
    a.o_rows = (double *)w.rows.p;
    a.o_lnprob = (double *)w.aux.p;
    a.o_index = (int *)(a.o_lnprob + nd);
    hipLaunchKernelGGL(k_draw_gather, dim3((unsigned)((nd + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    // the derived columns of the drawn rows alone: the compact block is a chain of nsrc x 1 x n, all of it the window
    mbb_summary_spec block = *sp->summary;
    block.burn = 0;
    block.thin = 1;
    mbbc::ChainView b;
    memset(&b, 0, sizeof b);
    fill_chain_view(b, a.o_rows, nsrc, 1, sp->n, &block, 16384);
    if ((rc = summary_fill_derived(c, &block, b))) return rc;
    HIPCHK(hipMemcpyAsync(o->rows, a.o_rows, nd * 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->lnprob, a.o_lnprob, nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->index, a.o_index, nd * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < 3; ++k)
        if (b.der[k]) HIPCHK(hipMemcpyAsync(o->derived[k], b.der[k], nd * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->status, c->der.colstatus.p, (size_t)nsrc * kCols * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = derived_sync(c))) return rc;
    for (int s = 0; s < nsrc; ++s)
        for (int k = 0; k < 3; ++k)
            if (!b.der[k]) o->status[(size_t)s * kCols + 5 + k] |= mbbs::kStAbsent;
    return MBB_OK;
}

extern "C" int mbb_chain_draws(mbb_ctx *c, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                               const mbb_draws_spec *spec, const mbb_draws_out *out)
{
    return analyse_chain(c, chain, lnprob, nsrc, nw, nsteps, [&] {
        return !chain ? fail(MBB_ERR_ARG, "bad arguments") : draws_check(nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *dl) { return draws_run(c, d, dl, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_draws(mbb_ctx *c, void *sp, const mbb_draws_spec *spec, const mbb_draws_out *out)
{
    return analyse_sampler(c, sp, spec && out, "drawn from", true, [&](const double *d, const double *dl, int nsrc, int nw, int nsteps) {
        return draws_run(c, d, dl, nsrc, nw, nsteps, spec, out);
    });
}

extern "C" int mbb_draw_indices(mbb_ctx *c, int nsrc, int nw, int nsteps, int burn, int thin, int n, int how,
                                unsigned long long seed, int32_t *index)
{
    using namespace mbbw;
    int rc = use(c);
    if (rc) return rc;
    if (!index) return fail(MBB_ERR_ARG, "null draws argument");
    mbb_summary_spec ss;
    memset(&ss, 0, sizeof ss);
    ss.burn = burn;
    ss.thin = thin;
    if ((rc = draws_check_picks(nsrc, nw, nsteps, &ss, n, how))) return rc;
    DrawArgs a;
    fill_draw_args(a, nullptr, nullptr, nsrc, nw, nsteps, &ss, n, how, seed);
    const size_t nd = (size_t)nsrc * n;
    if ((rc = grow(c, c->draw.aux, nd * 2 * sizeof(int)))) return rc;
    a.o_index = (int *)c->draw.aux.p;
    hipLaunchKernelGGL(k_draw_index, dim3((unsigned)((nd + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(index, a.o_index, nd * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

// ---- goodness of fit of a chain (mbb_goodness.hip.h) ------------------------
// What every goodness call needs of the context, and of the sources its rows belong to: before anything else is done.
static int good_check_ctx(const mbb_ctx *c, int nsrc)
{
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    if (c->data_nb <= 0) return fail(MBB_ERR_STATE, "data not set (mbb_set_data)");
    if (c->data_nb != c->nb) return fail(MBB_ERR_STATE, "the data and the bands differ in number");
    if (c->nb > mbbq::kMaxBands) return fail(MBB_ERR_ARG, "more than 256 bands in a goodness call");
    if (nsrc != c->nsrc && c->nsrc != 1)
        return fail(MBB_ERR_ARG, "the chain's sources must be the context's, or the context hold one source for all");
    return MBB_OK;
}

// The argument checks of a goodness call: before anything is allocated, uploaded or launched.
static int good_check(const mbb_ctx *c, int nsrc, int nw, int nsteps, const mbb_goodness_spec *sp, const mbb_goodness_out *o)
{
    if (!sp || !o || !o->n_used || !o->mean || !o->min || !o->max || !o->status || !o->pct || !o->at_mean || !o->ml ||
        !o->ml_index || !o->ml_model || !o->best || !o->best_index)
        return fail(MBB_ERR_ARG, "null goodness argument");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    int rc;
    if ((rc = good_check_ctx(c, nsrc))) return rc;
    if ((rc = check_percentiles(sp->npct, sp->pct, "1 to 8 percentiles per goodness call"))) return rc;
    if ((rc = check_burn_thin(sp->burn, sp->thin, nsteps))) return rc;
    if ((rc = check_sample_cap(sp->burn, sp->thin, nw, nsteps, "more than 2^32 - 1 samples per column"))) return rc;
    return check_grid((size_t)nsrc * 5);
}

// The context's bands on the device as the goodness kernels read them: samples, their logarithms, weights, the band table.
static int good_upload_bands(mbb_ctx *c, mbbq::FluxArgs &fa)
{
    mbb_ctx::GoodWork &w = c->good;
    const int nb = c->nb, ns = c->band_off[nb];
    int rc;
    if ((rc = grow(c, w.samples, (size_t)ns * 3 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.band, (size_t)nb * 3 * sizeof(int32_t)))) return rc;
    std::vector<int32_t> tab((size_t)nb * 3);
    memset(&fa, 0, sizeof fa);
    for (int b = 0; b < nb; ++b) {
        const int s0 = c->band_off[b], s1 = c->band_off[b + 1];
        const int single = s1 - s0 == 1 && c->band_wt[s0] == 1.0;
        tab[3 * b] = s0; tab[3 * b + 1] = s1; tab[3 * b + 2] = single;
        if (single) ++fa.nsingle; else ++fa.nmany;
    }
    double *const d_nu = (double *)w.samples.p, *const d_ln = d_nu + ns, *const d_wt = d_ln + ns;
    // (pageable sources: the copies have read them when they return)
    HIPCHK(hipMemcpyAsync(d_nu, c->band_freq.data(), (size_t)ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_wt, c->band_wt.data(), (size_t)ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(w.band.p, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(mbbq::k_good_lnnu, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream, (const double *)d_nu, ns, d_ln);
    HIPCHK(hipGetLastError());
    fa.nu = d_nu; fa.lnnu = d_ln; fa.wt = d_wt;
    fa.band = (const int32_t *)w.band.p;
    fa.nb = nb; fa.nsamples = ns;
    return MBB_OK;
}

// Band fluxes of the n rows whose records launch_prologue has just made: k_good_flux.
static int good_flux(mbb_ctx *c, mbbq::FluxArgs &fa, int n)
{
    using namespace mbbq;
    fa.wk = c->sed.wk.d(); fa.status = c->sed.status.d();
    fa.n = n; fa.mf = (double *)c->good.mf.p;
    const bool stage = fa.nmany > 0 && fa.nsamples <= kLdsSamples;
    const size_t lds = stage ? (size_t)fa.nsamples * 3 * sizeof(double) : 0;
    const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
    dispatch_variant(c->opthin, c->noalpha, [&](auto OT, auto NA) {
        if (stage)
            hipLaunchKernelGGL((k_good_flux<decltype(OT)::value, decltype(NA)::value, true>), grid, dim3(kThreads), lds, c->stream, fa);
        else
            hipLaunchKernelGGL((k_good_flux<decltype(OT)::value, decltype(NA)::value, false>), grid, dim3(kThreads), 0, c->stream, fa);
    });
    HIPCHK(hipGetLastError());
    return MBB_OK;
}

// Those band fluxes and the context's data as the kernel behind them reads both (mbbq::ChiArgs, mbbpw::GArgs: the same
// fields); returns the LDS bytes its launch needs for the covariance.
template <typename Args>
static size_t bind_data(const mbb_ctx *c, const mbbq::FluxArgs &fa, Args &a, int n)
{
    a.mf = fa.mf; a.status = fa.status; a.n = n; a.nb = c->nb;
    a.nsrc_data = c->nsrc;
    a.flux = c->data.flux.d(); a.ivar = c->data.ivar.d();
    a.invcov = c->has_cov ? c->data.invcov.d() : nullptr;
    a.cov_in_lds = c->has_cov && c->nb <= mbbq::kLdsCov;
    return a.cov_in_lds ? (size_t)c->nb * c->nb * sizeof(double) : 0;
}

// ... and their chisq and q: k_good_flux, then k_good_chi.  ca carries where the results go.
static int good_eval(mbb_ctx *c, mbbq::FluxArgs &fa, mbbq::ChiArgs &ca, int n)
{
    using namespace mbbq;
    if (const int rc = good_flux(c, fa, n)) return rc;
    const size_t clds = bind_data(c, fa, ca, n);
    hipLaunchKernelGGL(k_good_chi, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), clds, c->stream, ca);
    HIPCHK(hipGetLastError());
    return MBB_OK;
}

// Goodness of fit of a chain that is on the device in emcee's layout (lnprob may be null).  Synchronous; the results
// land in the caller's arrays.
static int good_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                    const mbb_goodness_spec *sp, const mbb_goodness_out *o)
{
    using namespace mbbq;
    int rc;
    if ((rc = good_check(c, nsrc, nw, nsteps, sp, o))) return rc;
    const int nb = c->nb;
    const size_t cells = (size_t)nsrc * nw * nsteps, s2 = (size_t)nsrc * 2, ns = (size_t)nsrc, np = (size_t)sp->npct;
    // theta-bar: the five parameter columns exactly as a summary of this window with neither clipping nor derived
    // columns reduces them
    mbb_summary_spec ss;
    memset(&ss, 0, sizeof ss);
    ss.burn = sp->burn; ss.thin = sp->thin;
    mbbs::SumArgs a5;
    memset(&a5, 0, sizeof a5);
    fill_chain_view(a5, d_chain, nsrc, nw, nsteps, &ss, 16384);
    // the two columns
    mbbs::SumArgs a;
    memset(&a, 0, sizeof a);
    fill_window_fixed(a, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    a.lnprob = d_lnprob;
    set_percentiles(a, sp->npct, sp->pct);
    a.ncol = 2; a.col[0] = 5; a.col[1] = 6;
    mbb_ctx::GoodWork &w = c->good;
    const size_t nev = 2 * ns;                              // rows evaluated at the end: theta-bar and the ML entry of every source
    const size_t rows_max = std::max(chunk_rows(cells), nev);
    FinishArgs f;
    PickArgs pk;
    double *ev_chisq, *ev_q, *ev_mf;                        // those rows' chisq, q and band fluxes [nev][nb], their status
    int *ev_status;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&f.o_nused, s2, o->n_used);
    rb.add(&f.o_mean, s2, o->mean); rb.add(&f.o_min, s2, o->min); rb.add(&f.o_max, s2, o->max);
    rb.add(&f.o_pct, s2 * np, o->pct);
    rb.add(&f.o_atmean, ns * 7, o->at_mean); rb.add(&f.o_ml, ns * 7, o->ml);
    rb.add(&pk.o_best, ns * 2, o->best);
    rb.add(&ev_chisq, nev); rb.add(&ev_q, nev);             // (the rows' chisq and q go home in at_mean and ml)
    rb.add(&ev_mf, nev * nb, o->ml_model, ns * nb);         // (theta-bar's band fluxes stay; the ML entries' go home)
    rb.add(&f.o_status, s2, o->status);
    rb.add(&pk.o_mlidx, ns * 2, o->ml_index); rb.add(&pk.o_bestidx, ns * 2, o->best_index);
    rb.add(&ev_status, nev);
    // (two views, theta-bar's five columns and the two columns, through the same part and state in stream order)
    if ((rc = grow_stats(c, ns * 5, a5.splits)) || (rc = grow_stats(c, s2, a.splits)) || (rc = grow_select(c, s2, a.splits))) return rc;
    if ((rc = grow(c, w.best, ns * a.splits * kBestWords * sizeof(double)))) return rc;
    if ((rc = grow(c, w.status, s2 * sizeof(int)))) return rc;
    if ((rc = grow(c, w.rows, nev * 5 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.mf, rows_max * nb * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    if ((rc = grow(c, c->der.der, 2 * cells * sizeof(double)))) return rc;
    if ((rc = ensure_sed(c, rows_max, 0))) return rc;
    double *const col0 = (double *)c->der.der.p, *const col1 = col0 + cells;
    a.der[0] = col0; a.der[1] = col1;
    a5.part = a.part = (double *)c->stat.part.p; a5.state = a.state = (mbbs::ColState *)c->stat.state.p;
    a.hist = (unsigned int *)c->stat.hist.p;
    double *const d_rows = (double *)w.rows.p;
    pk.o_ml = f.o_ml;
    f.gstatus = (const int *)w.status.p;
    f.tbar = d_rows; f.ev_chisq = ev_chisq; f.ev_q = ev_q;
    pk.part = (const double *)w.best.p; pk.ml_row = d_rows + ns * 5;
    FluxArgs fa;
    if ((rc = good_upload_bands(c, fa))) return rc;
    HIPCHK(hipMemsetAsync(w.status.p, 0, s2 * sizeof(int), c->stream));
    // theta-bar
    launch_stats(c, a5, ns * 5);
    hipLaunchKernelGGL(k_good_mean, dim3((unsigned)((ns * 5 + 63) / 64)), dim3(64), 0, c->stream, a5, d_rows);
    HIPCHK(hipGetLastError());
    // the columns, a chunk of rows at a time
    rc = for_row_chunks(c, d_chain, cells, c->wavenorm, [&](size_t off, int n) {
        ChiArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.off = ca.out = (long long)off; ca.rows_per_src = (long long)nw * nsteps;
        ca.chisq = col0; ca.q = col1;
        ca.gstatus = (int *)w.status.p; ca.nw = nw; ca.nsteps = nsteps; ca.burn = sp->burn; ca.thin = sp->thin;
        return good_eval(c, fa, ca, n);
    });
    if (rc) return rc;
    // their statistics, by the summary's kernels
    launch_stats(c, a, s2);
    launch_select(c, a, s2);
    // the maximum-likelihood and the maximum-lnprob entries
    hipLaunchKernelGGL(k_good_best, dim3((unsigned)nsrc, (unsigned)a.splits), dim3(kThreads), 0, c->stream, a, (double *)w.best.p);
    hipLaunchKernelGGL(k_good_pick, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, c->stream, a, pk);
    HIPCHK(hipGetLastError());
    // theta-bar and the ML entry of every source, evaluated as rows: row i belongs to source i mod nsrc
    {
        if ((rc = launch_prologue(c, d_rows, (int)nev, c->opthin, c->noalpha, c->wavenorm, 0, nullptr))) return rc;
        ChiArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.off = 0; ca.rows_per_src = 1;
        ca.chisq = ev_chisq; ca.q = ev_q; ca.row_status = ev_status; ca.mf_rows = ev_mf;
        if ((rc = good_eval(c, fa, ca, (int)nev))) return rc;
    }
    hipLaunchKernelGGL(k_good_finish, dim3((unsigned)((s2 + 63) / 64)), dim3(64), 0, c->stream, a, f);
    HIPCHK(hipGetLastError());
    return fetch_home(c, w.outbuf, rb);
}

extern "C" int mbb_chain_goodness(mbb_ctx *c, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                                  const mbb_goodness_spec *spec, const mbb_goodness_out *out)
{
    return analyse_chain(c, chain, lnprob, nsrc, nw, nsteps, [&] {
        return !chain ? fail(MBB_ERR_ARG, "bad arguments") : good_check(c, nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *dl) { return good_run(c, d, dl, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_goodness(mbb_ctx *c, void *sp, const mbb_goodness_spec *spec, const mbb_goodness_out *out)
{
    return analyse_sampler(c, sp, spec && out, "tested for goodness of fit", true,
                           [&](const double *d, const double *dl, int nsrc, int nw, int nsteps) {
        return good_run(c, d, dl, nsrc, nw, nsteps, spec, out);
    });
}

// The rows entries' shell (mbb_goodness_rows, mbb_pointwise_rows): n parameter rows of the context's sources, a chunk at
// a time -- their records by run_prologue, then eval(fa, off, m, chunk) evaluates rows [off, off + m) and enqueues the
// copies out of outbuf (null with a null context), which holds per row of a chunk a double per band and extra_bytes.
template <typename Eval>
static int eval_rows(mbb_ctx *c, const double *pars, int n, bool args_ok, DevBuf *outbuf, size_t extra_bytes, Eval &&eval)
{
    int rc = use(c);
    if (rc) return rc;
    if (!pars || n <= 0 || !args_ok) return fail(MBB_ERR_ARG, "bad arguments");
    if ((rc = good_check_ctx(c, c->nsrc))) return rc;
    if (n % c->nsrc != 0) return fail(MBB_ERR_ARG, "in multi-source mode the rows must be nsources equal blocks");
    const size_t chunk = std::min<size_t>((size_t)n, (size_t)kSumChunkRows);
    if ((rc = grow(c, c->good.mf, chunk * c->nb * sizeof(double)))) return rc;
    if ((rc = grow(c, *outbuf, chunk * (c->nb * sizeof(double) + extra_bytes)))) return rc;
    if ((rc = ensure_sed(c, chunk, 0))) return rc;
    mbbq::FluxArgs fa;
    if ((rc = good_upload_bands(c, fa))) return rc;
    for (size_t off = 0; off < (size_t)n; off += chunk) {
        const int m = (int)std::min(chunk, (size_t)n - off);
        if ((rc = run_prologue(c, pars + off * 5, m, c->opthin, c->noalpha, c->wavenorm, 0, nullptr))) return rc;
        if ((rc = eval(fa, off, m, chunk))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return MBB_OK;
}

extern "C" int mbb_goodness_rows(mbb_ctx *c, const double *pars, int n, double *chisq, double *q, int32_t *status,
                                 double *model_flux)
{
    using namespace mbbq;
    return eval_rows(c, pars, n, chisq && q && status, c ? &c->good.outbuf : nullptr, 2 * sizeof(double) + sizeof(int),
                     [&](FluxArgs &fa, size_t off, int m, size_t chunk) -> int {
        const int nb = c->nb;
        Carve ob{(char *)c->good.outbuf.p};
        double *const d_chisq = ob.take<double>(chunk), *const d_q = ob.take<double>(chunk), *const d_mf = ob.take<double>(chunk * nb);
        int *const d_status = ob.take<int>(chunk);
        ChiArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.off = (long long)off; ca.rows_per_src = n / c->nsrc;
        ca.chisq = d_chisq; ca.q = d_q; ca.row_status = d_status; ca.mf_rows = model_flux ? d_mf : nullptr;
        if (const int rc = good_eval(c, fa, ca, m)) return rc;
        HIPCHK(hipMemcpyAsync(chisq + off, d_chisq, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(q + off, d_q, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status + off, d_status, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (model_flux)
            HIPCHK(hipMemcpyAsync(model_flux + off * nb, d_mf, (size_t)m * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        return MBB_OK;
    });
}

// ---- out-of-sample fit of a chain (mbb_pointwise.hip.h) -----------------------
// The argument checks of a pointwise call: before anything is allocated, uploaded or launched.
static int pw_check(const mbb_ctx *c, int nsrc, int nw, int nsteps, const mbb_pointwise_spec *sp, const mbb_pointwise_out *o)
{
    if (!sp || !o || !o->n_used || !o->tail_len || !o->status || !o->lppd || !o->p_waic || !o->elpd_waic || !o->elpd_loo ||
        !o->p_loo || !o->khat || !o->loo_pit)
        return fail(MBB_ERR_ARG, "null pointwise argument");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    int rc;
    if ((rc = good_check_ctx(c, nsrc))) return rc;
    if ((rc = check_burn_thin(sp->burn, sp->thin, nsteps))) return rc;
    const long long kept = kept_steps(sp->burn, sp->thin, nsteps);
    if ((long long)nw * kept > MBB_PW_MAX_WINDOW || mbbps::ps_tail_len((long long)nw * kept) > mbbps::kTailMax)
        return fail(MBB_ERR_ARG, "the window's tail would be longer than one workgroup sorts (MBB_PW_MAX_WINDOW entries per source)");
    return check_grid((size_t)nsrc * c->nb);
}

// k_pw_g on the band fluxes good_flux has just made of n rows.  ga carries where the results go and the group.
static int pw_g(mbb_ctx *c, const mbbq::FluxArgs &fa, mbbpw::GArgs &ga, int n)
{
    const size_t clds = bind_data(c, fa, ga, n);
    hipLaunchKernelGGL(mbbpw::k_pw_g, dim3((unsigned)((n + mbbq::kThreads - 1) / mbbq::kThreads)), dim3(mbbq::kThreads), clds,
                       c->stream, ga);
    HIPCHK(hipGetLastError());
    return MBB_OK;
}

// WAIC and PSIS-LOO of a chain that is on the device in emcee's layout.  Synchronous; the results land in the caller's
// arrays.  The bands are worked on a group at a time: two columns of the chain's length per band of a group.
static int pw_run(mbb_ctx *c, const double *d_chain, int nsrc, int nw, int nsteps, const mbb_pointwise_spec *sp,
                  const mbb_pointwise_out *o)
{
    using namespace mbbpw;
    int rc;
    if ((rc = pw_check(c, nsrc, nw, nsteps, sp, o))) return rc;
    const int nb = c->nb;
    const size_t cells = (size_t)nsrc * nw * nsteps, ns = (size_t)nsrc, tab = ns * nb;
    const long long budget = (c->opt.pw_budget_mb > 0 ? c->opt.pw_budget_mb : 0) * (1ll << 20);
    const int group = (int)std::max<long long>(1, std::min<long long>(nb, budget / (long long)(2 * cells * sizeof(double))));
    PwArgs a;
    memset(&a, 0, sizeof a);
    fill_window_fixed(a, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    a.nb = nb; a.cells = (long long)cells;
    a.ivar = c->data.ivar.d(); a.invcov = c->has_cov ? c->data.invcov.d() : nullptr; a.nsrc_data = c->nsrc;
    mbb_ctx::PwWork &w = c->pw;
    mbb_ctx::GoodWork &gw = c->good;
    const size_t chunk = chunk_rows(cells);
    const size_t nsel = (size_t)((group + kSelCols - 1) / kSelCols) * ns * kSelCols;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&a.o_nused, tab, o->n_used);
    rb.add(&a.o_lppd, tab, o->lppd); rb.add(&a.o_pwaic, tab, o->p_waic); rb.add(&a.o_elpdwaic, tab, o->elpd_waic);
    rb.add(&a.o_elpdloo, tab, o->elpd_loo); rb.add(&a.o_ploo, tab, o->p_loo); rb.add(&a.o_khat, tab, o->khat);
    rb.add(&a.o_pit, tab, o->loo_pit);
    rb.add(&a.o_tail, tab, o->tail_len); rb.add(&a.o_status, tab, o->status);
    if ((rc = grow(c, w.cols, (size_t)group * 2 * cells * sizeof(double)))) return rc;
    if ((rc = grow(c, w.part, ns * group * a.splits * (kPartWords + 1) * sizeof(double)))) return rc;
    if ((rc = grow(c, w.state, ns * group * sizeof(PwState)))) return rc;
    if ((rc = grow(c, w.sel, nsel * sizeof(mbbs::ColState)))) return rc;
    if ((rc = grow_select(c, ns * kSelCols, a.splits))) return rc;
    if ((rc = grow(c, w.status, ns * sizeof(int)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    if ((rc = grow(c, gw.mf, chunk * nb * sizeof(double)))) return rc;
    if ((rc = ensure_sed(c, chunk, 0))) return rc;
    a.gcol = (double *)w.cols.p; a.lwcol = a.gcol + (size_t)group * cells;
    a.part = (double *)w.part.p; a.part2 = a.part + ns * group * a.splits * kPartWords;
    a.state = (PwState *)w.state.p; a.sel = (mbbs::ColState *)w.sel.p;
    a.gstatus = (const int *)w.status.p;
    mbbq::FluxArgs fa;
    if ((rc = good_upload_bands(c, fa))) return rc;
    HIPCHK(hipMemsetAsync(w.status.p, 0, ns * sizeof(int), c->stream));
    for (int b0 = 0; b0 < nb; b0 += group) {
        a.b0 = b0; a.ng = std::min(group, nb - b0);
        // g of the group's bands, a chunk of rows at a time: one band-flux fill per group
        rc = for_row_chunks(c, d_chain, cells, c->wavenorm, [&](size_t off, int n) -> int {
            if (const int rf = good_flux(c, fa, n)) return rf;
            GArgs ga;
            memset(&ga, 0, sizeof ga);
            ga.off = (long long)off; ga.rows_per_src = (long long)nw * nsteps;
            ga.b0 = b0; ga.ng = a.ng; ga.gcol = a.gcol; ga.cells = (long long)cells;
            ga.gstatus = b0 == 0 ? (int *)w.status.p : nullptr;
            ga.nw = nw; ga.nsteps = nsteps; ga.burn = sp->burn; ga.thin = sp->thin;
            return pw_g(c, fa, ga, n);
        });
        if (rc) return rc;
        const size_t ncid = ns * a.ng;
        const dim3 gcol((unsigned)ncid, (unsigned)a.splits);
        hipLaunchKernelGGL(k_pw_stat1, gcol, dim3(kThreads), 0, c->stream, a);
        hipLaunchKernelGGL(k_pw_begin, dim3((unsigned)((ncid + 63) / 64)), dim3(64), 0, c->stream, a);
        hipLaunchKernelGGL(k_pw_stat2, gcol, dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
        // the cutoffs, by the summary's select: kSelCols bands of the group per launch, as its derived columns
        for (int q = 0; q * kSelCols < a.ng; ++q) {
            mbbs::SumArgs s;
            memset(&s, 0, sizeof s);
            static_cast<mbbc::ChainView &>(s) = static_cast<const mbbc::ChainView &>(a);
            s.ncol = std::min(kSelCols, a.ng - q * kSelCols);
            for (int k = 0; k < s.ncol; ++k) { s.col[k] = 5 + k; s.der[k] = a.lwcol + (size_t)(q * kSelCols + k) * cells; }
            s.state = a.sel + (size_t)q * ns * kSelCols;
            s.hist = (unsigned int *)c->stat.hist.p;
            launch_select(c, s, ns * s.ncol);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_pw_tail, dim3((unsigned)ncid), dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    return fetch_home(c, w.outbuf, rb);
}

extern "C" int mbb_chain_pointwise(mbb_ctx *c, const double *chain, int nsrc, int nw, int nsteps,
                                   const mbb_pointwise_spec *spec, const mbb_pointwise_out *out)
{
    return analyse_chain(c, chain, nullptr, nsrc, nw, nsteps, [&] { return pw_check(c, nsrc, nw, nsteps, spec, out); },
                         [&](const double *d, const double *) { return pw_run(c, d, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_pointwise(mbb_ctx *c, void *sp, const mbb_pointwise_spec *spec, const mbb_pointwise_out *out)
{
    return analyse_sampler(c, sp, spec && out, "cross-validated", false, [&](const double *d, const double *, int nsrc, int nw, int nsteps) {
        return pw_run(c, d, nsrc, nw, nsteps, spec, out);
    });
}

extern "C" int mbb_pointwise_rows(mbb_ctx *c, const double *pars, int n, double *ll, int32_t *status)
{
    return eval_rows(c, pars, n, ll && status, c ? &c->pw.outbuf : nullptr, sizeof(int),
                     [&](mbbq::FluxArgs &fa, size_t off, int m, size_t chunk) -> int {
        const int nb = c->nb;
        Carve ob{(char *)c->pw.outbuf.p};
        double *const d_ll = ob.take<double>(chunk * nb);
        int *const d_status = ob.take<int>(chunk);
        int rc;
        if ((rc = good_flux(c, fa, m))) return rc;
        mbbpw::GArgs ga;
        memset(&ga, 0, sizeof ga);
        ga.off = (long long)off; ga.rows_per_src = n / c->nsrc;
        ga.b0 = 0; ga.ng = nb; ga.ll_rows = d_ll; ga.row_status = d_status;
        if ((rc = pw_g(c, fa, ga, m))) return rc;
        HIPCHK(hipMemcpyAsync(ll + off * nb, d_ll, (size_t)m * nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(status + off, d_status, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        return MBB_OK;
    });
}

// ---- a chain reweighted under another density (mbb_reweight.hip.h) -------------
static_assert(mbbrw::kStKHigh == MBB_RW_K_HIGH && mbbrw::kStTailShort == MBB_RW_TAIL_SHORT &&
              mbbrw::kStTailFlat == MBB_RW_TAIL_FLAT && mbbrw::kStHasZero == MBB_RW_HAS_ZERO &&
              mbbrw::kStAllZero == MBB_RW_ALL_ZERO, "the header's status bits are the kernels'");
static_assert(mbbrw::kStKHigh == mbbpw::kStKHigh && mbbrw::kStTailShort == mbbpw::kStTailShort &&
              mbbrw::kStTailFlat == mbbpw::kStTailFlat, "the Pareto bits are the out-of-sample fit's");
static_assert(mbbrw::kMaxPct == MBB_SUMMARY_MAX_PCT && mbbrw::kCols == MBB_SUMMARY_COLS, "the summary's sizes");
static_assert((long long)mbbrws::kUnit == MBB_RW_WEIGHT_ONE &&(double)MBB_PW_MAX_WINDOW * (double)MBB_RW_WEIGHT_ONE < 9007199254740992.0,
              "a window's weights sum below 2^53");
static_assert(mbbps::kTailMax == MBB_PW_TAIL_MAX, "the tail one workgroup sorts");

// The argument checks of a reweighting: before anything is allocated, uploaded or launched.  c is the target.
static int rw_check(const mbb_ctx *c, int nsrc, int nw, int nsteps, const mbb_reweight_spec *sp, const mbb_reweight_out *o)
{
    if (!sp || !o || !sp->summary || !o->n_used || !o->n_zero || !o->n_left_out || !o->weight_sum || !o->khat || !o->ess ||
        !o->lnz_ratio || !o->mean || !o->pct || !o->cov || !o->best || !o->tail_len || !o->status || !o->col_status ||
        !o->best_index)
        return fail(MBB_ERR_ARG, "null reweight argument");
    if (sharded_context(c))
        return fail(MBB_ERR_STATE, "a sharded context cannot reweight a chain: a rank holds only its own walkers' chain");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    if (c->data_nb != c->nb) return fail(MBB_ERR_STATE, "data not set or band count mismatch");
    if (nsrc != c->nsrc && c->nsrc != 1)
        return fail(MBB_ERR_ARG, "the chain's sources must be the target's, or the target hold one source for all");
    const mbb_summary_spec *ss = sp->summary;
    int rc;
    if ((rc = check_percentiles(ss->npct, ss->pct, "1 to 8 percentiles per reweighting"))) return rc;
    if ((rc = check_window(ss, nsteps))) return rc;
    const long long n = (long long)nw * kept_steps(ss->burn, ss->thin, nsteps);
    if (n > MBB_PW_MAX_WINDOW)
        return fail(MBB_ERR_ARG, "the window's weights would not sum below 2^53, nor its tail fit one workgroup (MBB_PW_MAX_WINDOW entries per source)");
    if ((rc = check_derived_settings(ss, nsrc))) return rc;
    if ((unsigned long long)nsrc * (unsigned long long)n / mbbrw::kThreads > 0x7fffffffull) return fail(MBB_ERR_ARG, "too many sources");
    return check_grid((size_t)nsrc * mbbrw::kCols);
}

// The chain on the device in emcee's layout, with its lnprob, reweighted under the density of c, the target: every work
// buffer is c's, every launch on c's stream.  Synchronous; the results land in the caller's arrays.
static int rw_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                  const mbb_reweight_spec *sp, const mbb_reweight_out *o)
{
    using namespace mbbrw;
    int rc;
    if ((rc = rw_check(c, nsrc, nw, nsteps, sp, o))) return rc;
    if (!d_lnprob) return fail(MBB_ERR_ARG, "a reweighting needs the chain's lnprob");
    const mbb_summary_spec *ss = sp->summary;
    RwArgs a;
    memset(&a, 0, sizeof a);
    fill_chain_view(a, d_chain, nsrc, nw, nsteps, ss, 16384);
    a.lnprob = d_lnprob;
    a.smooth = sp->smooth != 0;
    a.npct = ss->npct;
    for (int k = 0; k < ss->npct; ++k) a.pct[k] = ss->pct[k];
    const size_t cells = (size_t)nsrc * nw * nsteps, ns = (size_t)nsrc, n = (size_t)a.n, sc = ns * kCols;
    const size_t ncolumns = ns * a.ncol, np = (size_t)ss->npct;
    // a slab: entries [k m, (k + 1) m) of every source, [nsrc][m][5] -- the likelihood's multi-source row grouping
    const size_t m = std::min<size_t>(n, std::max<size_t>(1, (size_t)kSumChunkRows / ns));
    const size_t srows = ns * m;
    mbb_ctx::RwWork &w = c->rw;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&a.o_nused, ns, o->n_used); rb.add(&a.o_nzero, ns, o->n_zero); rb.add(&a.o_nleft, ns, o->n_left_out);
    rb.add(&a.o_wsum, ns, o->weight_sum);
    rb.add(&a.o_khat, ns, o->khat); rb.add(&a.o_ess, ns, o->ess); rb.add(&a.o_lnz, ns, o->lnz_ratio);
    rb.add(&a.o_mean, sc, o->mean); rb.add(&a.o_pct, sc * np, o->pct);
    rb.add(&a.o_cov, ns * 25, o->cov); rb.add(&a.o_best, ns * 6, o->best);
    rb.add(&a.o_tail, ns, o->tail_len); rb.add(&a.o_status, ns, o->status); rb.add(&a.o_colstatus, sc, o->col_status);
    rb.add(&a.o_bestidx, ns * 2, o->best_index);
    const bool entries = o->target_lnprob || o->log_ratio || o->log_weight || o->weight;
    if ((rc = grow(c, w.slab, srows * (6 * sizeof(double) + sizeof(int32_t))))) return rc;
    if ((rc = grow(c, w.cols, cells * 3 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.count, ns * a.splits * kCountWords * sizeof(unsigned long long)))) return rc;
    if ((rc = grow(c, w.state, ns * sizeof(RwState)))) return rc;
    if ((rc = grow(c, w.sel, ns * sizeof(mbbs::ColState)))) return rc;
    if ((rc = grow_select(c, ns, a.splits))) return rc;
    if ((rc = grow(c, w.status, ns * sizeof(int)))) return rc;
    if ((rc = grow(c, w.wpart, ncolumns * a.splits * kWStatWords * sizeof(double)))) return rc;
    if ((rc = grow(c, w.wstate, ncolumns * sizeof(WColState)))) return rc;
    if ((rc = grow(c, w.whist, ncolumns * a.splits * kMaxPct * 256 * sizeof(unsigned long long)))) return rc;
    if ((rc = grow(c, w.covpart, ns * a.splits * kCovWords * sizeof(double)))) return rc;
    if (entries && (rc = grow(c, w.entries, ns * n * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.lqcol = (double *)w.cols.p; a.lwcol = a.lqcol + cells;
    a.ucol = (unsigned long long *)(a.lwcol + cells);
    a.count = (unsigned long long *)w.count.p;
    a.state = (RwState *)w.state.p; a.sel = (mbbs::ColState *)w.sel.p;
    a.gstatus = (int *)w.status.p;
    a.wpart = (double *)w.wpart.p; a.wstate = (WColState *)w.wstate.p; a.whist = (unsigned long long *)w.whist.p;
    a.covpart = (double *)w.covpart.p;
    Carve sb{(char *)w.slab.p};
    a.s_rows = sb.take<double>(srows * 5);
    double *const s_lnl = sb.take<double>(srows);
    int32_t *const s_status = sb.take<int32_t>(srows);
    a.s_lnl = s_lnl; a.s_status = s_status;
    HIPCHK(hipMemsetAsync(w.status.p, 0, ns * sizeof(int), c->stream));
    // the target's lnprob of the window's rows, a slab at a time
    for (size_t i0 = 0; i0 < n; i0 += m) {
        const size_t mm = std::min(m, n - i0), rows = ns * mm;
        a.i0 = (long long)i0; a.m = (int)mm;
        const dim3 grid((unsigned)((rows + kThreads - 1) / kThreads));
        hipLaunchKernelGGL(k_rw_gather, grid, dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
        if ((rc = launch_rows(c, a.s_rows, (int)rows, s_lnl, s_status, nullptr))) return rc;
        hipLaunchKernelGGL(k_rw_ratio, grid, dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
    }
    // the log weights
    const dim3 gsrc((unsigned)nsrc, (unsigned)a.splits);
    hipLaunchKernelGGL(k_rw_count, gsrc, dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_rw_begin, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(k_rw_shift, gsrc, dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    {
        // the cutoff, by the summary's select: the lw column as its first derived column
        mbbs::SumArgs s;
        memset(&s, 0, sizeof s);
        static_cast<mbbc::ChainView &>(s) = static_cast<const mbbc::ChainView &>(a);
        s.ncol = 1; s.col[0] = 5; s.der[0] = a.lwcol; s.der[1] = s.der[2] = nullptr;
        s.state = a.sel;
        s.hist = (unsigned int *)c->stat.hist.p;
        launch_select(c, s, ns);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rw_tail, dim3((unsigned)nsrc), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    // the weighted statistics of the summary's columns
    if ((rc = summary_fill_derived(c, ss, a))) return rc;
    a.colstatus = (const int *)c->der.colstatus.p;
    const dim3 gcol((unsigned)ncolumns, (unsigned)a.splits);
    hipLaunchKernelGGL(k_rw_wstats, gcol, dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_rw_wbegin, dim3((unsigned)((ncolumns + 63) / 64)), dim3(64), 0, c->stream, a);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(k_rw_whist, gcol, dim3(kThreads), 0, c->stream, a, pass);
        hipLaunchKernelGGL(k_rw_wpick, dim3((unsigned)ncolumns), dim3(kThreads), 0, c->stream, a);
    }
    hipLaunchKernelGGL(k_rw_cov, gsrc, dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_rw_finish, dim3((unsigned)((sc + 63) / 64)), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    if ((rc = fetch_image(c, w.outbuf, rb)) || (rc = derived_sync(c))) return rc;
    rb.scatter();
    // the per-entry outputs asked for, one after the other through one block
    void *const dst[4] = {o->target_lnprob, o->log_ratio, o->log_weight, o->weight};
    for (int what = 0; what < 4; ++what) {
        if (!dst[what]) continue;
        hipLaunchKernelGGL(k_rw_entries, dim3((unsigned)((ns * n + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                           a, what, (double *)w.entries.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(dst[what], w.entries.p, ns * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return MBB_OK;
}

extern "C" int mbb_chain_reweight(mbb_ctx *target, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                                  const mbb_reweight_spec *spec, const mbb_reweight_out *out)
{
    return analyse_chain(target, chain, lnprob, nsrc, nw, nsteps, [&] {
        if (!chain || !lnprob) return fail(MBB_ERR_ARG, "bad arguments: a reweighting needs the chain and its lnprob");
        return rw_check(target, nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *dl) { return rw_run(target, d, dl, nsrc, nw, nsteps, spec, out); });
}

// c owns the sampler and the resident chain; target, the same context or another of this process and device, owns the
// work.  c's stream is brought to rest before target's first launch; rw_run leaves target's at rest.
extern "C" int mbb_sampler_reweight(mbb_ctx *c, void *sp, mbb_ctx *target, const mbb_reweight_spec *spec,
                                    const mbb_reweight_out *out)
{
    if (!target) return fail(MBB_ERR_ARG, "null reweight argument");
    return analyse_sampler(c, sp, spec && out, "reweighted", true,
                           [&](const double *d, const double *dl, int nsrc, int nw, int nsteps) -> int {
        int rc;
        if (target->device != c->device) return fail(MBB_ERR_ARG, "the target context is on another device than the chain");
        if (sharded_context(c))
            return fail(MBB_ERR_STATE, "a sharded context cannot reweight a chain: a rank holds only its own walkers' chain");
        if ((rc = rw_check(target, nsrc, nw, nsteps, spec, out))) return rc;
        if (target != c && (rc = use(target))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        return rw_run(target, d, dl, nsrc, nw, nsteps, spec, out);
    });
}

// ---- the population of a catalogue (mbb_population.hip.h) ----------------------
static_assert(mbbpop::kStEmpty == MBB_SUM_EMPTY && mbbpop::kStHasNan == MBB_SUM_HAS_NAN &&
              mbbpop::kCandBad == MBB_POP_CAND_BAD && mbbpop::kCandUnderflow == MBB_POP_CAND_UNDERFLOW &&
              mbbpop::kCandHasEmpty == MBB_POP_CAND_HAS_EMPTY, "the header's status bits are the kernels'");
static_assert(mbbpop::kMaxCand == MBB_POP_MAX_CAND && mbbpops::kIdentity == MBB_POP_IDENTITY &&
              mbbpops::kLog10 == MBB_POP_LOG10, "the header's constants are the kernels'");
static_assert(mbbpop::kChunk % mbbpop::kTile == 0 && mbbpop::kChunk % mbbpop::kTileMom == 0 &&
              mbbpop::kChunk % mbbpop::kTileMomWide == 0, "a launch holds whole tiles");

// The argument checks of a population build: before anything is allocated, uploaded or launched.
static int pop_check(const mbb_ctx *c, int nsrc, int nw, int nsteps, const mbb_population_spec *sp,
                     const mbb_population_build_out *o)
{
    if (!sp || !o || !o->n_used || !o->n_left_out || !o->status || !o->serial)
        return fail(MBB_ERR_ARG, "null population argument");
    if (sharded_context(c))
        return fail(MBB_ERR_STATE, "a sharded context cannot pool a chain into a population: a rank holds only its own walkers' chain");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    if (sp->d < 1 || sp->d > mbbpops::kMaxD) return fail(MBB_ERR_ARG, "a population has 1 to 5 columns");
    unsigned seen = 0;
    for (int i = 0; i < sp->d; ++i) {
        if (sp->col[i] < 0 || sp->col[i] > 4) return fail(MBB_ERR_ARG, "unknown population column: the five parameters are 0 to 4");
        if ((seen >> sp->col[i]) & 1u) return fail(MBB_ERR_ARG, "a population column is given twice");
        seen |= 1u << sp->col[i];
        if (sp->transform[i] != MBB_POP_IDENTITY && sp->transform[i] != MBB_POP_LOG10)
            return fail(MBB_ERR_ARG, "unknown population transform");
    }
    if (const int rc = check_burn_thin(sp->burn, sp->thin, nsteps)) return rc;
    const unsigned long long n = (unsigned long long)nw * (unsigned long long)kept_steps(sp->burn, sp->thin, nsteps);
    const unsigned long long bps = (n + mbbpop::kThreads - 1) / mbbpop::kThreads;
    if (bps * (unsigned long long)nsrc > 0x7fffffffull) return fail(MBB_ERR_ARG, "too many sources");
    return check_grid((size_t)nsrc);
}

// A population block that cannot be made: the allocator's status, and what to do about it.
static int pop_alloc_failed(mbb_ctx *c, int rc)
{
    c->pop.x.release(); c->pop.b.release();
    g_err = "the population block cannot be allocated (" + g_err + "): thin the window";
    return rc;
}

// The window of the chain on the device into the context's block.  Synchronous.
static int pop_build(mbb_ctx *c, const double *d_chain, int nsrc, int nw, int nsteps, const mbb_population_spec *sp,
                     const mbb_population_build_out *o)
{
    using namespace mbbpop;
    int rc;
    if ((rc = pop_check(c, nsrc, nw, nsteps, sp, o))) return rc;
    mbb_ctx::PopBlock &w = c->pop;
    w.live = false;
    const long long serial = ++w.serial;
    PopBuildArgs a;
    memset(&a, 0, sizeof a);
    fill_window(a, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    a.d = sp->d;
    for (int i = 0; i < sp->d; ++i) { a.pcol[i] = sp->col[i]; a.transform[i] = sp->transform[i]; }
    for (int k = 0; k < 5; ++k) {
        a.prior.has_uplim[k] = sp->has_uplim[k] != 0; a.prior.has_gprior[k] = sp->has_gprior[k] != 0;
        a.prior.lowlim[k] = sp->lowlim[k]; a.prior.uplim[k] = sp->uplim[k];
        a.prior.gmean[k] = sp->gmean[k]; a.prior.givar[k] = sp->givar[k];
    }
    const size_t ns = (size_t)nsrc, n = (size_t)a.n;
    if ((rc = grow(c, w.x, ns * n * sp->d * sizeof(double))) || (rc = grow(c, w.b, ns * n * sizeof(double))))
        return pop_alloc_failed(c, rc);
    if ((rc = grow(c, w.count, ns * sizeof(unsigned long long)))) return rc;
    ResultBlock rb;
    rb.add(&a.o_nused, ns, o->n_used); rb.add(&a.o_nleft, ns, o->n_left_out); rb.add(&a.o_status, ns, o->status);
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.x = (double *)w.x.p; a.b = (double *)w.b.p; a.count = (unsigned long long *)w.count.p;
    a.blocks_per_src = (unsigned)((n + kThreads - 1) / kThreads);
    HIPCHK(hipMemsetAsync(w.count.p, 0, ns * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_pop_build, dim3((unsigned)(ns * a.blocks_per_src)), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_pop_status, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    if ((rc = fetch_home(c, w.outbuf, rb))) return rc;
    w.nsrc = nsrc; w.d = sp->d; w.n = a.n;
    // the splits of a source's entries: a function of n alone
    w.splits = (int)std::min<long long>(kMaxSplits, (a.n + kSplitEntries - 1) / kSplitEntries);
    w.per_split = (a.n + w.splits - 1) / w.splits;
    w.live = true;
    *o->serial = serial;
    return MBB_OK;
}

extern "C" int mbb_chain_population_build(mbb_ctx *c, const double *chain, int nsrc, int nw, int nsteps,
                                          const mbb_population_spec *spec, const mbb_population_build_out *out)
{
    return analyse_chain(c, chain, nullptr, nsrc, nw, nsteps, [&] { return pop_check(c, nsrc, nw, nsteps, spec, out); },
                         [&](const double *d, const double *) { return pop_build(c, d, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_population_build(mbb_ctx *c, void *sp, const mbb_population_spec *spec,
                                            const mbb_population_build_out *out)
{
    return analyse_sampler(c, sp, spec && out, "pooled into a population", false,
                           [&](const double *d, const double *, int nsrc, int nw, int nsteps) {
        return pop_build(c, d, nsrc, nw, nsteps, spec, out);
    });
}

template <int D, bool MOM> static void pop_launch(mbb_ctx *c, const mbbpop::PopEvalArgs &a)
{
    using namespace mbbpop;
    constexpr int TILE = pop_tile(D, MOM);
    const dim3 grid((unsigned)a.nsrc, (unsigned)a.splits, (unsigned)((a.hn + TILE - 1) / TILE));
    hipLaunchKernelGGL((k_pop_eval<D, MOM>), grid, dim3(kThreads), 0, c->stream, a);
    const long long pairs = (long long)a.hn * a.nsrc;
    hipLaunchKernelGGL((k_pop_merge<D, MOM>), dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, c->stream, a);
}

template <int D> static void pop_launch_d(mbb_ctx *c, const mbbpop::PopEvalArgs &a)
{
    if (a.moments) pop_launch<D, true>(c, a); else pop_launch<D, false>(c, a);
}

extern "C" int mbb_population_eval(mbb_ctx *c, int64_t serial, const double *hyper, int H, int moments,
                                   const mbb_population_eval_out *o)
{
    using namespace mbbpop;
    int rc = use(c);
    if (rc) return rc;
    if (!hyper || !o || !o->lnl || !o->n_src_used || !o->cand_status || (moments && (!o->mean || !o->cov)))
        return fail(MBB_ERR_ARG, "null population argument");
    if (H < 1 || H > MBB_POP_MAX_CAND) return fail(MBB_ERR_ARG, "a population evaluation takes 1 to MBB_POP_MAX_CAND (1024) candidates");
    if (sharded_context(c))
        return fail(MBB_ERR_STATE, "a sharded context cannot pool a chain into a population: a rank holds only its own walkers' chain");
    mbb_ctx::PopBlock &w = c->pop;
    if (!w.live || serial != (int64_t)w.serial)
        return fail(MBB_ERR_STATE, "no population block of this serial in the context: it was replaced by a later build, or dropped");
    const int d = w.d, hl = mbbpops::pop_hyper_len(d);
    const size_t ns = (size_t)w.nsrc, nh = (size_t)H, pairs = nh * ns;
    const int words = 3 + (moments ? d + mbbpops::pop_tri(d) : 0);
    PopEvalArgs a;
    memset(&a, 0, sizeof a);
    ResultBlock rb;
    rb.add(&a.o_lnl, nh, o->lnl);
    rb.add(&a.lnl_src, pairs, o->lnl_src); rb.add(&a.ess, pairs, o->ess);
    rb.add(&a.mean, moments ? pairs * d : 0, moments ? o->mean : nullptr);
    rb.add(&a.cov, moments ? pairs * d * d : 0, moments ? o->cov : nullptr);
    rb.add(&a.o_nsrc_used, nh, o->n_src_used); rb.add(&a.o_cand_status, nh, o->cand_status);
    const size_t chunk = std::min<size_t>(nh, kChunk);
    if ((rc = grow(c, w.hyper, nh * hl * sizeof(double)))) return rc;
    if ((rc = grow(c, w.part, chunk * ns * w.splits * words * sizeof(double)))) return rc;
    if ((rc = place(c, w.lsrc, rb))) return rc;
    HIPCHK(hipMemcpyAsync(w.hyper.p, hyper, nh * hl * sizeof(double), hipMemcpyHostToDevice, c->stream));
    a.x = (const double *)w.x.p; a.b = (const double *)w.b.p; a.count = (const unsigned long long *)w.count.p;
    a.hyper = (const double *)w.hyper.p;
    a.nsrc = w.nsrc; a.d = d; a.H = H; a.n = w.n; a.per_split = w.per_split; a.splits = w.splits; a.moments = moments != 0;
    a.part = (double *)w.part.p;
    for (int h0 = 0; h0 < H; h0 += kChunk) {
        a.h0 = h0; a.hn = std::min(kChunk, H - h0);
        switch (d) {
        case 1: pop_launch_d<1>(c, a); break;
        case 2: pop_launch_d<2>(c, a); break;
        case 3: pop_launch_d<3>(c, a); break;
        case 4: pop_launch_d<4>(c, a); break;
        default: pop_launch_d<5>(c, a); break;
        }
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pop_total, dim3((unsigned)H), dim3(64), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    // what the caller asked for goes home, entry by entry: the [H][nsrc] tables stay on the device when it did not
    rc = rb.each([&](void *dst, size_t off, size_t bytes) -> int {
        HIPCHK(hipMemcpyAsync(dst, (const char *)w.lsrc.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
        return MBB_OK;
    });
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

extern "C" int mbb_population_drop(mbb_ctx *c)
{
    int rc = use(c);
    if (rc) return rc;
    if ((rc = sync_stream(c))) return rc;
    mbb_ctx::PopBlock &w = c->pop;
    w.live = false;
    w.x.release(); w.b.release(); w.count.release(); w.hyper.release(); w.part.release(); w.lsrc.release(); w.outbuf.release();
    return MBB_OK;
}

// ---- the maximum of the posterior (mbb_map.hip.h) ------------------------------
// The argument checks of mbb_map_fit: before anything is allocated, uploaded or launched.
static int map_check(const mbb_ctx *c, const mbb_map_spec *sp, const mbb_map_out *o)
{
    if (!sp || !o) return fail(MBB_ERR_ARG, "null map argument");
    if (!sp->start || !o->params || !o->lnprob || !o->chisq || !o->q || !o->cov || !o->niter || !o->nfev ||
        !o->start_index || !o->status)
        return fail(MBB_ERR_ARG, "null map argument");
    if (sharded_context(c))
        return fail(MBB_ERR_STATE, "a sharded context cannot run a map fit: every rank would repeat the whole search");
    if (sp->nsrc < 1) return fail(MBB_ERR_ARG, "a map fit needs a source at least");
    if (c->nb > mbbmap::kMaxBands) return fail(MBB_ERR_ARG, "more than 256 bands in a map fit");
    if (sp->nsrc != c->nsrc && c->nsrc != 1)
        return fail(MBB_ERR_ARG, "the starts' sources must be the context's, or the context hold one source for all");
    int rc;
    if ((rc = good_check_ctx(c, sp->nsrc))) return rc;
    if (sp->nstart < 1 || sp->nstart > MBB_MAP_MAX_STARTS) return fail(MBB_ERR_ARG, "1 to 64 starts per source");
    if (sp->maxiter < 1 || sp->maxiter > MBB_MAP_MAX_ITER) return fail(MBB_ERR_ARG, "1 to 1000 iterations per map fit");
    if (!(sp->ftol >= 0.0 && sp->ftol <= 1.7976931348623157e308) || !(sp->xtol >= 0.0 && sp->xtol <= 1.7976931348623157e308))
        return fail(MBB_ERR_ARG, "ftol and xtol must be finite and not negative");
    if ((rc = check_grid((size_t)sp->nsrc * sp->nstart))) return rc;
    const size_t nval = (size_t)sp->nsrc * sp->nstart * 5;
    for (size_t i = 0; i < nval; ++i)
        if (!(fabs(sp->start[i]) <= 1.7976931348623157e308)) {
            char buf[96];
            snprintf(buf, sizeof buf, "start of source %zu, start %zu is not finite", i / 5 / sp->nstart, i / 5 % sp->nstart);
            return fail(MBB_ERR_ARG, buf);
        }
    return MBB_OK;
}

extern "C" int mbb_map_fit(mbb_ctx *c, const mbb_map_spec *sp, const mbb_map_out *o)
{
    using namespace mbbmap;
    int rc = use(c);
    if (rc) return rc;
    if ((rc = map_check(c, sp, o))) return rc;
    const int nb = c->nb, nsrc = sp->nsrc, nstart = sp->nstart;
    const size_t n = (size_t)nsrc * nstart;
    mbb_ctx::MapWork &w = c->map;
    MapArgs a;
    memset(&a, 0, sizeof a);
    ResultBlock rb;                              // (the host reads both in place from the image: nothing is scattered)
    const size_t at_d = rb.add(&a.outd, n * kOutDoubles), at_i = rb.add(&a.outi, n * kOutInts);
    if ((rc = grow(c, w.start, n * 5 * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    mbbq::FluxArgs fa;
    if ((rc = good_upload_bands(c, fa))) return rc;
    HIPCHK(hipMemcpyAsync(w.start.p, sp->start, n * 5 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    a.start = (const double *)w.start.p; a.nstart = nstart; a.nsrc_data = c->nsrc;
    a.nu = fa.nu; a.lnnu = fa.lnnu; a.wt = fa.wt; a.band = fa.band; a.nb = nb; a.nsamples = fa.nsamples;
    a.flux = c->data.flux.d(); a.ivar = c->data.ivar.d();
    a.invcov = c->has_cov ? c->data.invcov.d() : nullptr;
    a.cov_in_lds = c->has_cov && nb <= kLdsCov;
    a.nunorm = kUmToGHz / c->wavenorm; a.lnunorm = log(kUmToGHz / c->wavenorm);
    for (int i = 0; i < 5; ++i) a.lowlim[i] = c->lowlim[i];
    for (int i = 0; i < 6; ++i) { a.uplim[i] = c->uplim[i]; a.gmean[i] = c->gmean[i]; a.givar[i] = c->givar[i]; }
    a.has_uplim = c->has_uplim; a.has_gprior = c->has_gprior;
    a.fixed = fixed_mask(c, sp->fixed);
    a.maxiter = sp->maxiter; a.ftol = sp->ftol; a.xtol = sp->xtol;
    const bool stage = fa.nmany > 0 && fa.nsamples <= kLdsSamples;
    const size_t lds = lds_doubles(nb, fa.nsamples, stage, c->has_cov != 0, a.cov_in_lds != 0) * sizeof(double);
    const int inst = model_of(c) * 2 + (stage ? 1 : 0);
    rc = MBB_OK;
    dispatch_variant(c->opthin, c->noalpha, [&](auto OT, auto NA) {
        auto launch = [&](auto kern) {
            if (lds > 56 * 1024 && !w.lds_granted[inst]) {
                // (beyond 64 KB of LDS per workgroup, the kernel's static LDS included, its dynamic-LDS ceiling has to be
                // raised.  The attribute is the function's, not the context's: every context asks for the same value, the
                // most a map fit can need, so that none can lower what another relies on)
                const size_t want = 152 * 1024;
                const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want);
                if (e != hipSuccess) { rc = fail(MBB_ERR_HIP, "hipFuncSetAttribute(k_map_lm)", e); return; }
                w.lds_granted[inst] = want;
            }
            hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(kThreads), lds, c->stream, a);
        };
        if (stage) launch(k_map_lm<decltype(OT)::value, decltype(NA)::value, true>);
        else launch(k_map_lm<decltype(OT)::value, decltype(NA)::value, false>);
    });
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    if ((rc = fetch_home(c, w.outbuf, rb))) return rc;
    const double *hd = (const double *)(rb.image() + at_d);
    const int32_t *hi = (const int32_t *)(rb.image() + at_i);
    // the final points of every (source, start) through the likelihood's own batch path: [nsrc][nstart][5] is its
    // multi-source layout, and the reported lnprob is what like(params) gives, bit for bit
    std::vector<double> pall(n * 5), lall(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) pall[i * 5 + k] = hd[i * kOutDoubles + k];
    if ((rc = mbb_lnlike_batch(c, pall.data(), (int)n, lall.data(), nullptr, nullptr))) return rc;
    // per source the start of largest lnprob: ties to the lowest index, a NaN never wins
    std::vector<double> picked((size_t)nsrc * 5);
    for (int s = 0; s < nsrc; ++s) {
        int best = -1;
        for (int j = 0; j < nstart; ++j) {
            const double v = lall[(size_t)s * nstart + j];
            if (v != v) continue;
            if (best < 0 || v > lall[(size_t)s * nstart + best]) best = j;
        }
        if (best < 0) best = 0;
        const size_t i = (size_t)s * nstart + best;
        for (int k = 0; k < 5; ++k) o->params[(size_t)s * 5 + k] = picked[(size_t)s * 5 + k] = pall[i * 5 + k];
        for (int k = 0; k < 25; ++k) o->cov[(size_t)s * 25 + k] = hd[i * kOutDoubles + 6 + k];
        o->lnprob[s] = lall[i];
        o->niter[s] = hi[i * kOutInts]; o->nfev[s] = hi[i * kOutInts + 1]; o->status[s] = hi[i * kOutInts + 2];
        o->start_index[s] = best;
    }
    if (o->lnprob_all) memcpy(o->lnprob_all, lall.data(), n * sizeof(double));
    if (o->params_all) memcpy(o->params_all, pall.data(), n * 5 * sizeof(double));
    if (o->status_all) for (size_t i = 0; i < n; ++i) o->status_all[i] = hi[i * kOutInts + 2];
    // the picked points through the goodness of fit's own path: its chisq, q and band fluxes
    std::vector<int32_t> gst((size_t)nsrc);
    return mbb_goodness_rows(c, picked.data(), nsrc, o->chisq, o->q, gst.data(), o->model_flux);
}

// ---- the evidence of a chain (mbb_evidence.hip.h) ------------------------------
static_assert(mbbev::kMaxN2 == MBB_EV_MAX_N2 && mbbev::kMaxIter == MBB_EV_MAX_ITER, "the header's limits are the kernels'");
static_assert(mbbev::kConverged == MBB_EV_CONVERGED && mbbev::kMaxIterHit == MBB_EV_MAXITER &&
              mbbev::kCovSingular == MBB_EV_COV_SINGULAR && mbbev::kPostLeftOut == MBB_EV_POST_LEFT_OUT &&
              mbbev::kNoOverlap == MBB_EV_NO_OVERLAP && mbbev::kAllHeld == MBB_EV_ALL_HELD &&
              mbbev::kHeldShift == MBB_EV_HELD_SHIFT, "the header's status bits are the kernels'");
// The argument checks of an evidence call: before anything is allocated, uploaded or launched.
static int ev_check(const mbb_ctx *c, int nsrc, int nw, int nsteps, const mbb_evidence_spec *sp, const mbb_evidence_out *o)
{
    if (!sp || !o || !o->lnz || !o->lnz_err || !o->niter || !o->status || !o->n1 || !o->n2_inside || !o->prop_mean ||
        !o->prop_cov)
        return fail(MBB_ERR_ARG, "null evidence argument");
    if (sharded_context(c))
        return fail(MBB_ERR_STATE, "a sharded context cannot estimate an evidence: a rank holds only its own walkers' chain");
    if (nsrc < 1 || nw < 1 || nsteps < 1) return fail(MBB_ERR_ARG, "empty chain");
    int rc;
    if ((rc = good_check_ctx(c, nsrc))) return rc;
    if ((rc = check_burn_thin(sp->burn, sp->thin, nsteps))) return rc;
    const long long nkept = kept_steps(sp->burn, sp->thin, nsteps);
    if (nkept < 2) return fail(MBB_ERR_ARG, "an evidence needs two kept steps at least: one half fits the proposal, the other is bridged to");
    if (sp->n2 < 0 || sp->n2 > MBB_EV_MAX_N2) return fail(MBB_ERR_ARG, "0 to 2^22 proposal draws per source");
    if ((long long)nw * nkept > 0x7fffffffll) return fail(MBB_ERR_ARG, "more than 2^31 - 1 samples per source");
    if (sp->n2 == 0 && (long long)nw * (nkept - nkept / 2) > MBB_EV_MAX_N2)
        return fail(MBB_ERR_ARG, "n2 = 0 asks for as many draws as posterior samples: more than 2^22, name n2");
    if (!(sp->tol >= 0.0 && sp->tol <= 1.7976931348623157e308)) return fail(MBB_ERR_ARG, "tol must be finite and not negative");
    if (sp->maxiter < 1 || sp->maxiter > MBB_EV_MAX_ITER) return fail(MBB_ERR_ARG, "1 to 100000 iterations per evidence");
    if (sp->first_source < 0) return fail(MBB_ERR_ARG, "first_source must not be negative");
    if ((rc = check_grid((size_t)nsrc))) return rc;
    if (sp->neff)
        for (int s = 0; s < nsrc; ++s)
            if (!(sp->neff[s] > 0.0 && sp->neff[s] <= 1.7976931348623157e308))
                return fail(MBB_ERR_ARG, "neff must be finite and positive");
    return MBB_OK;
}

// The evidence of a chain that is on the device in emcee's layout, with its lnprob.  Synchronous; the results land in
// the caller's arrays.
static int evidence_run(mbb_ctx *c, const double *d_chain, const double *d_lnprob, int nsrc, int nw, int nsteps,
                        const mbb_evidence_spec *sp, const mbb_evidence_out *o)
{
    using namespace mbbev;
    int rc;
    if ((rc = ev_check(c, nsrc, nw, nsteps, sp, o))) return rc;
    if (!d_lnprob) return fail(MBB_ERR_ARG, "an evidence needs the chain's lnprob");
    EvArgs a;
    memset(&a, 0, sizeof a);
    fill_window(a, d_chain, nsrc, nw, nsteps, sp->burn, sp->thin);
    a.lnprob = d_lnprob;
    a.nfit = a.nkept / 2; a.n1k = a.nkept - a.nfit;
    a.n1max = (long long)nw * a.n1k;
    a.n2 = sp->n2 ? sp->n2 : (int)a.n1max;
    a.fixed = fixed_mask(c, sp->fixed);
    a.first_source = sp->first_source; a.seed = sp->seed; a.tol = sp->tol; a.maxiter = sp->maxiter;
    const size_t ns = (size_t)nsrc, n1 = (size_t)a.n1max, n2 = (size_t)a.n2;
    // a slab: draws [k m, (k + 1) m) of every source, [nsrc][m][5] -- the likelihood's multi-source row grouping
    const size_t m = std::min<size_t>(n2, std::max<size_t>(1, (size_t)kSumChunkRows / ns));
    const size_t srows = ns * m;
    mbb_ctx::EvWork &w = c->ev;
    ResultBlock rb;                              // 64-bit counts, doubles, 32-bit words
    rb.add(&a.o_n1, ns, o->n1); rb.add(&a.o_inside, ns, o->n2_inside);
    rb.add(&a.o_lnz, ns, o->lnz); rb.add(&a.o_err, ns, o->lnz_err);
    rb.add(&a.o_niter, ns, o->niter);
    if ((rc = grow(c, w.mom, ns * kMomWords * sizeof(double)))) return rc;
    if ((rc = grow(c, w.ints, ns * 2 * sizeof(int)))) return rc;
    if ((rc = grow(c, w.slab, srows * (7 * sizeof(double) + sizeof(int32_t))))) return rc;
    if ((rc = grow(c, w.l1, ns * n1 * sizeof(double)))) return rc;
    if ((rc = grow(c, w.l2, ns * n2 * sizeof(double)))) return rc;
    if (o->post_lnq && (rc = grow(c, w.postq, ns * n1 * sizeof(double)))) return rc;
    if (sp->neff && (rc = grow(c, w.neff, ns * sizeof(double)))) return rc;
    if ((rc = place(c, w.outbuf, rb))) return rc;
    a.mom = (double *)w.mom.p;
    a.free_ = (int *)w.ints.p; a.status = a.free_ + ns;
    a.l1 = (double *)w.l1.p; a.l2 = (double *)w.l2.p;
    a.post_lnq = o->post_lnq ? (double *)w.postq.p : nullptr;
    Carve sb{(char *)w.slab.p};
    a.s_rows = sb.take<double>(srows * 5); a.s_lnq = sb.take<double>(srows);
    double *const s_lnl = sb.take<double>(srows);
    int32_t *const s_status = sb.take<int32_t>(srows);
    a.s_lnl = s_lnl;
    if (sp->neff) {
        // (a pageable source: the copy has read it when it returns)
        HIPCHK(hipMemcpyAsync(w.neff.p, sp->neff, ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
        a.neff = (const double *)w.neff.p;
    }
    hipLaunchKernelGGL(k_ev_moments, dim3((unsigned)nsrc), dim3(kThreads), 0, c->stream, a);
    hipLaunchKernelGGL(k_ev_factor, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, c->stream, a);
    hipLaunchKernelGGL(k_ev_post, dim3((unsigned)((ns * n1 + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    for (size_t i0 = 0; i0 < n2; i0 += m) {
        const size_t mm = std::min(m, n2 - i0), rows = ns * mm;
        a.i0 = (int)i0; a.m = (int)mm;
        const dim3 grid((unsigned)((rows + kThreads - 1) / kThreads));
        hipLaunchKernelGGL(k_ev_propose, grid, dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
        if ((rc = launch_rows(c, a.s_rows, (int)rows, s_lnl, s_status, nullptr))) return rc;
        hipLaunchKernelGGL(k_ev_l2, grid, dim3(kThreads), 0, c->stream, a);
        HIPCHK(hipGetLastError());
        // the slab's rows, lnP and lnq into the caller's [nsrc][N2] arrays where asked for
        if (o->prop)
            HIPCHK(hipMemcpy2DAsync(o->prop + i0 * 5, n2 * 5 * sizeof(double), a.s_rows, mm * 5 * sizeof(double),
                                    mm * 5 * sizeof(double), ns, hipMemcpyDeviceToHost, c->stream));
        if (o->prop_lnprob)
            HIPCHK(hipMemcpy2DAsync(o->prop_lnprob + i0, n2 * sizeof(double), s_lnl, mm * sizeof(double),
                                    mm * sizeof(double), ns, hipMemcpyDeviceToHost, c->stream));
        if (o->prop_lnq)
            HIPCHK(hipMemcpy2DAsync(o->prop_lnq + i0, n2 * sizeof(double), a.s_lnq, mm * sizeof(double),
                                    mm * sizeof(double), ns, hipMemcpyDeviceToHost, c->stream));
        if (o->prop || o->prop_lnprob || o->prop_lnq) HIPCHK(hipStreamSynchronize(c->stream));   // (before the slab is reused)
    }
    hipLaunchKernelGGL(k_ev_bridge, dim3((unsigned)nsrc), dim3(kThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    std::vector<double> mom(ns * kMomWords);
    if ((rc = fetch_image(c, w.outbuf, rb))) return rc;
    HIPCHK(hipMemcpyAsync(mom.data(), w.mom.p, mom.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(o->status, a.status, ns * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (o->post_lnq)
        HIPCHK(hipMemcpyAsync(o->post_lnq, w.postq.p, ns * n1 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    rb.scatter();
    for (size_t s = 0; s < ns; ++s) {
        memcpy(o->prop_mean + s * 5, &mom[s * kMomWords + kMomMean], 5 * sizeof(double));
        memcpy(o->prop_cov + s * 25, &mom[s * kMomWords + kMomCov], 25 * sizeof(double));
    }
    return MBB_OK;
}

extern "C" int mbb_chain_evidence(mbb_ctx *c, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                                  const mbb_evidence_spec *spec, const mbb_evidence_out *out)
{
    return analyse_chain(c, chain, lnprob, nsrc, nw, nsteps, [&] {
        if (!chain || !lnprob) return fail(MBB_ERR_ARG, "bad arguments: an evidence needs the chain and its lnprob");
        return ev_check(c, nsrc, nw, nsteps, spec, out);
    }, [&](const double *d, const double *dl) { return evidence_run(c, d, dl, nsrc, nw, nsteps, spec, out); });
}

extern "C" int mbb_sampler_evidence(mbb_ctx *c, void *sp, const mbb_evidence_spec *spec, const mbb_evidence_out *out)
{
    return analyse_sampler(c, sp, spec && out, "bridged to an evidence", true,
                           [&](const double *d, const double *dl, int nsrc, int nw, int nsteps) {
        return evidence_run(c, d, dl, nsrc, nw, nsteps, spec, out);
    });
}

// Measurement helper: the empirical roof of the sample arithmetic (k_roof).
extern "C" int mbb_roof_probe(mbb_ctx *c, const double pars[5], int reps, double *seconds,
                              double *lane_slots, double *clock_mhz)
{
    int rc = use(c);
    if (rc) return rc;
    if (!pars || reps <= 0 || !seconds || !lane_slots) return fail(MBB_ERR_ARG, "bad arguments");
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    const int threads = c->opt.roof_threads > 0 ? (int)c->opt.roof_threads : 512;
    const int grid = (int)(c->opt.roof_wgs > 0 ? c->opt.roof_wgs : 2) * c->cu_count;
    if ((rc = ensure_sed(c, 1, (size_t)grid * threads + 2))) return rc;
    if ((rc = run_prologue(c, pars, 1, c->opthin, c->noalpha, c->wavenorm, 0, nullptr))) return rc;
    unsigned long long *d_clk = reinterpret_cast<unsigned long long *>(c->sed.out.d() + (size_t)grid * threads);
    LikeArgs a;
    memset(&a, 0, sizeof a);
    a.nu = c->band.nu.d(); a.lnnu = c->band.lnnu.d(); a.wt = c->band.wt.d();
    a.poly_b = c->d_poly_b; a.poly_c = c->d_poly_c;
    a.nchunk = c->nchunk;
    EventPair ev;
    if ((rc = ev.create())) return rc;
    const hipEvent_t e0 = ev.e[0], e1 = ev.e[1];
    for (int pass = 0; pass < 2; ++pass) {            // the first pass warms clocks and caches
        HIPCHK(hipEventRecord(e0, c->stream));
        dispatch_variant(c->opthin, c->noalpha, [&](auto OT, auto NA) {
            hipLaunchKernelGGL((k_roof<decltype(OT)::value, decltype(NA)::value>), dim3(grid), dim3(threads),
                               0, c->stream, a, c->sed.wk.d(), reps, c->sed.out.d(), d_clk);
        });
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
    }
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *seconds = ms * 1e-3;
    *lane_slots = (double)grid * (threads / 64) * (double)reps * c->nchunk * 64.0;
    if (clock_mhz) {
        unsigned long long clk[2] = {0, 0};
        HIPCHK(hipMemcpy(clk, d_clk, sizeof clk, hipMemcpyDeviceToHost));
        *clock_mhz = clk[1] ? 100.0 * (double)clk[0] / (double)clk[1] : 0.0;
    }
    return MBB_OK;
}

extern "C" int mbb_fnu_eval(mbb_ctx *c, int opthin, int noalpha, const double *freq, int n,
                            double T, double beta, double x0, double alpha, double normfac,
                            double xmerge, double kappa, double *out)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || !freq || !out) return fail(MBB_ERR_ARG, "bad arguments");
    if ((rc = ensure_sed(c, 1, (size_t)2 * n))) return rc;
    double *d_freq = c->sed.out.d() + n;
    HIPCHK(hipMemcpyAsync(d_freq, freq, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const int threads = 256, grid = (n + threads - 1) / threads;
    dispatch_variant(opthin, noalpha, [&](auto OT, auto NA) {
        hipLaunchKernelGGL((k_fnu_explicit<decltype(OT)::value, decltype(NA)::value>), dim3(grid),
                           dim3(threads), 0, c->stream, d_freq, n, T, beta, x0, alpha, normfac,
                           xmerge, kappa, c->sed.out.d());
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->sed.out.d(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}

// ---- plumbing ---------------------------------------------------------------
extern "C" int mbb_malloc(mbb_ctx *c, size_t bytes, void **dptr)
{
    int rc = use(c);
    if (rc) return rc;
    if (!dptr) return fail(MBB_ERR_ARG, "null dptr");
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 1));
    return MBB_OK;
}
extern "C" int mbb_free(mbb_ctx *c, void *dptr)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    if (dptr) HIPCHK(hipFree(dptr));
    return MBB_OK;
}
extern "C" int mbb_memcpy_h2d(mbb_ctx *c, void *dst, const void *src, size_t bytes)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}
extern "C" int mbb_memcpy_d2h(mbb_ctx *c, void *dst, const void *src, size_t bytes)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}
extern "C" int mbb_sync(mbb_ctx *c)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return MBB_OK;
}
extern "C" void *mbb_stream(mbb_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" int mbb_event_create(mbb_ctx *c, void **ev)
{
    int rc = use(c);
    if (rc) return rc;
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    *ev = (void *)e;
    return MBB_OK;
}
extern "C" int mbb_event_record(mbb_ctx *c, void *ev)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipEventRecord((hipEvent_t)ev, c->stream));
    return MBB_OK;
}
extern "C" int mbb_event_elapsed_ms(mbb_ctx *c, void *start, void *stop, float *ms)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipEventSynchronize((hipEvent_t)stop));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return MBB_OK;
}
extern "C" int mbb_event_destroy(mbb_ctx *c, void *ev)
{
    int rc = use(c);
    if (rc) return rc;
    HIPCHK(hipEventDestroy((hipEvent_t)ev));
    return MBB_OK;
}

#ifdef MBB_STAMPS
extern "C" int mbb_stamps(mbb_ctx *c, unsigned long long *host, int nblocks)
{
    int rc = use(c);
    if (rc) return rc;
    if (!c->stamps.p) {
        if ((rc = c->stamps.remake(32 * sizeof(unsigned long long) * 65536))) return rc;
        HIPCHK(hipMemset(c->stamps.d(), 0, 32 * sizeof(unsigned long long) * 65536));
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mbbd::g_pstamps), &c->stamps.p, sizeof(c->stamps.p)));
    }
    if (host) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(host, c->stamps.d(), 32 * sizeof(unsigned long long) * nblocks, hipMemcpyDeviceToHost));
    }
    return MBB_OK;
}
#endif

extern "C" int mbb_set_option(mbb_ctx *c, const char *name, long value)
{
    if (!c || !name) return fail(MBB_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> own(c->srv_mu);
    if (c->serving) {                               // (a resident server runs with the options of its launch)
        HIPCHK(hipSetDevice(c->device));
        int rc = serve_stop(c);
        if (rc) return rc;
    }
    c->srv_hot = 0;
    const mbbopt::OptionRow *row = mbbopt::set_option(c->opt, name, value);
    if (!row) return fail(MBB_ERR_ARG, "unknown option");
    if (row->field == &mbbopt::Options::serve) { c->srv_strikes = 0; c->srv_rest = 0; }
    if (row->field == &mbbopt::Options::serve_after) c->srv_need = 0;
    return MBB_OK;
}

// What mbb_get_info answers, by name; the keys a sampler's run asks for at every call come first.
struct InfoRow {
    const char *name;
    long (*get)(mbb_ctx *);
};
#define INFO(name, value) {name, [](mbb_ctx *c) -> long { return value; }}
static const InfoRow kInfo[] = {
    INFO("nranks", c->x.connected ? c->x.n : c->nranks),
    INFO("rank", c->x.connected ? c->x.rank : c->rank),
    INFO("flow_fallbacks", c->flow_fallbacks),
    INFO("flow_resting", c->flow_rest),
    INFO("nb", c->nb),
    INFO("nseg", c->nseg),
    INFO("nunit", c->nunit),
    INFO("last_prep_ns", c->t_prep_ns),
    INFO("serving", c->serving ? 1 : 0),
    INFO("serve_requests", c->srv_requests),
    INFO("serve_fallbacks", c->srv_fallbacks),
    INFO("last_prepass", c->last_prepass),
    INFO("serve_enabled", c->opt.serve),
    INFO("device_peers", mbbh::registry_peers(c->reg_key, true)),
    INFO("serve_peer_yields", c->srv_peer_yields),
    INFO("serve_resizes", c->srv_resizes),
    INFO("serve_rests", c->srv_rests),
    INFO("serve_resting", c->srv_rest),
    INFO("device_busy", c->srv_busy),
    INFO("serve_grid", c->serving ? c->srv_grid : 0),
    INFO("serve_lease_yields", c->srv_lease_yields),
    INFO("last_launch_ns", c->t_launch_ns),
    INFO("last_wait_ns", c->t_wait_ns),
    INFO("last_watch_seen", c->last_watch_seen),
    INFO("simd_chunks_max", *std::max_element(c->simd_chunks, c->simd_chunks + 4)),
    INFO("simd_chunks_min", *std::min_element(c->simd_chunks, c->simd_chunks + 4)),
    INFO("nchunk", c->nchunk),
    INFO("nq", c->nq),
    INFO("cu_count", c->cu_count),
    INFO("last_wpb", c->last_wpb),
    INFO("last_threads", c->last_threads),
    INFO("last_grid", c->last_grid),
    INFO("last_kernel_form", c->last_smode),     // k_lnlike's SMODE of the last launch
    INFO("last_workgroups_ahead", c->last_ahead),
    INFO("last_smem", c->last_smem),
    INFO("last_stage", c->last_stage),
    INFO("device", c->device),
    INFO("xchg_launches", (long)c->x.seq),
};
#undef INFO

extern "C" int mbb_get_info(mbb_ctx *c, const char *name, long *value)
{
    if (!c || !name || !value) return fail(MBB_ERR_ARG, "null argument");
    for (const InfoRow &r : kInfo)
        if (!strcmp(name, r.name)) {
            *value = r.get(c);
            return MBB_OK;
        }
    return fail(MBB_ERR_ARG, "unknown info key");
}

// ---- one-hop exchange between the ranks of a sharded sampler run ----------------
// (the direct exchange on the xGMI mesh instead of a ring
// collective for a 6 KB message.)  Replaces emcee's pool, mbb_fit.py:80-81.
// "xchg_spin_max" is the exchange's: it goes back to its default with every close.
static void xchg_close(mbb_ctx *c)
{
    c->x.close();
    c->opt.xchg_spin_max = mbbopt::Options().xchg_spin_max;
}

extern "C" int mbb_xchg_open(mbb_ctx *c, int nranks, int rank, int max_rows, unsigned char handle[64])
{
    int rc = use(c);
    if (rc) return rc;
    if (nranks < 1 || nranks > 16 || rank < 0 || rank >= nranks || max_rows <= 0 || !handle)
        return fail(MBB_ERR_ARG, "bad exchange layout (at most 16 ranks)");
    if (c->x.base.p) return fail(MBB_ERR_STATE, "this context already has an exchange (mbb_xchg_close first)");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "handle size");
    const size_t bytes = mbb_ctx::Xchg::kHeader + (size_t)max_rows * 6 * sizeof(double) +
                         spec_words((size_t)max_rows) * sizeof(double);
    // fine-grained: peers' system-scope stores must be visible to this device's loads while
    // kernels run on both sides
    // (an exchange that does not get as far as its handle is closed again: nothing half-made stays with the context)
    if ((rc = c->x.base.remake(bytes))) return rc;
    hipIpcMemHandle_t h;
    hipError_t e = hipMemset(c->x.base.d(), 0, bytes);
    const char *what = "hipMemset(c->x.base, 0, bytes)";
    if (e == hipSuccess) { e = hipDeviceSynchronize(); what = "hipDeviceSynchronize()"; }
    if (e == hipSuccess) { e = hipIpcGetMemHandle(&h, c->x.base.d()); what = "hipIpcGetMemHandle"; }
    if (e != hipSuccess) { xchg_close(c); return fail(MBB_ERR_HIP, what, e); }
    memcpy(handle, &h, 64);
    c->x.n = nranks; c->x.rank = rank; c->x.cap_rows = (size_t)max_rows; c->x.connected = 0; c->x.seq = 0;
    c->x.peer[rank] = c->x.base.d();
    return MBB_OK;
}

// handles: nranks x 64 bytes, entry r as returned by rank r's mbb_xchg_open (entry `rank` is ignored).
// Every rank must have returned from mbb_xchg_open before any calls this.
extern "C" int mbb_xchg_connect(mbb_ctx *c, const unsigned char *handles)
{
    int rc = use(c);
    if (rc) return rc;
    if (!c->x.base.p || !handles) return fail(MBB_ERR_STATE, "mbb_xchg_open first");
    if (c->x.connected) return fail(MBB_ERR_STATE, "exchange already connected");
    for (int r = 0; r < c->x.n; ++r) {
        if (r == c->x.rank) continue;
        hipIpcMemHandle_t h;
        memcpy(&h, handles + (size_t)r * 64, 64);
        void *p = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) return fail(MBB_ERR_HIP, "hipIpcOpenMemHandle", e);
        c->x.peer[r] = (unsigned char *)p;
    }
    if ((rc = c->x.d_args.remake(sizeof(XchgArgs))) || (rc = c->x.d_flowx.remake(sizeof(FlowX)))) return rc;
    c->x.connected = 1;
    return MBB_OK;
}

extern "C" int mbb_xchg_close(mbb_ctx *c)
{
    int rc = use(c);
    if (rc) return rc;
    if (c->x.users > 0) return fail(MBB_ERR_STATE, "a sampler still lives in the exchange buffer (mbb_sampler_destroy first)");
    HIPCHK(hipStreamSynchronize(c->stream));
    xchg_close(c);
    return MBB_OK;
}

// ---- RCCL -------------------------------------------------------------------
extern "C" int mbb_comm_unique_id(char id[128])
{
    int rc = load_rccl();
    if (rc) return rc;
    UniqueId u;
    memset(&u, 0, sizeof u);
    int r = g_rccl.GetUniqueId(&u);
    if (r != 0) return fail(MBB_ERR_RCCL, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "ncclGetUniqueId failed");
    memcpy(id, u.internal, 128);
    return MBB_OK;
}

extern "C" int mbb_comm_init(mbb_ctx *c, int nranks, int rank, const char id[128])
{
    int rc = use(c);
    if (rc) return rc;
    if (nranks < 1 || rank < 0 || rank >= nranks || !id) return fail(MBB_ERR_ARG, "bad rank layout");
    if (c->comm) return fail(MBB_ERR_STATE, "this context already has a communicator (mbb_comm_destroy first)");
    if ((rc = load_rccl())) return rc;
    UniqueId u;
    memcpy(u.internal, id, 128);
    int r = g_rccl.CommInitRank(&c->comm, nranks, u, rank);
    if (r != 0) return fail(MBB_ERR_RCCL, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "ncclCommInitRank failed");
    c->nranks = nranks;
    c->rank = rank;
    return MBB_OK;
}

extern "C" int mbb_comm_destroy(mbb_ctx *c)
{
    int rc = use(c);
    if (rc) return rc;
    if (c->comm) {
        HIPCHK(hipStreamSynchronize(c->stream));
        g_rccl.CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->nranks = 1;
    c->rank = 0;
    return MBB_OK;
}

extern "C" int mbb_allgather_f64(mbb_ctx *c, const double *d_send, double *d_recv, int count);

// One sharded half-step in one call: this rank's n walkers through the fused
// kernel, then the all-gather of their log-probabilities, both on the context's
// stream.  d_all holds nranks*n doubles, rank-major; d_lnl is this rank's slice
// of d_all (in-place all-gather) or a separate buffer.
extern "C" int mbb_lnlike_allgather_device(mbb_ctx *c, const double *d_pars, int n, double *d_lnl,
                                           int32_t *d_status, double *d_all)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || !d_pars || !d_lnl || !d_all) return fail(MBB_ERR_ARG, "bad batch buffers");
    if ((rc = launch_rows(c, d_pars, n, d_lnl, d_status, nullptr))) return rc;
    return mbb_allgather_f64(c, d_lnl, d_all, n);
}

// The sharded boundary as ONE call, host arrays in and out (what emcee's pool does per half-step,
// mbb_fit.py:80-81: every worker evaluates its share of the rows, everybody gets all the answers): this
// rank's n parameter rows go to the device without a copy command (through the BAR, or read by the kernel
// from pinned memory), the fused kernel writes its lnprob into this rank's slice of the gather buffer and
// its row status straight into pinned host memory, ONE in-place ncclAllGather of n doubles per rank, one
// copy of the nranks*n gathered values to a pinned landing buffer, one stream wait.
extern "C" int mbb_lnlike_allgather(mbb_ctx *c, const double *pars, int n, double *all, int32_t *status)
{
    int rc = use(c);
    if (rc) return rc;
    if (n <= 0 || !pars || !all) return fail(MBB_ERR_ARG, "bad batch buffers");
    if (c->nb <= 0) return fail(MBB_ERR_STATE, "bands not set (mbb_set_bands)");
    const int nranks = c->comm ? c->nranks : 1, rank = c->comm ? c->rank : 0;
    if (!c->comm && c->nranks != 1) return fail(MBB_ERR_STATE, "communicator not initialised");
    if ((rc = ensure_capacity(c, (size_t)n, false))) return rc;
    const size_t total = (size_t)nranks * n;
    {
        size_t cap = c->gather.d.cap ? c->gather.d.cap : 1024 * sizeof(double);
        while (cap < total * sizeof(double)) cap *= 2;
        if ((rc = grow(c, c->gather.d, cap)) || (rc = grow(c, c->gather.h, cap))) return rc;
    }
    const size_t nbytes = (size_t)n * 5 * sizeof(double);
    const bool push = c->opt.zero_copy && c->opt.bar_params && c->bnd.w_pars.d();
    double *dp;
    int32_t *ds;
    if (push) {
        memcpy(c->bnd.w_pars.d(), pars, nbytes);
        __builtin_ia32_sfence();
        dp = c->bnd.w_pars.d();
    } else {
        memcpy(c->bnd.h_pars.h(), pars, nbytes);
        if (c->opt.zero_copy) dp = c->bnd.h_pars.dv();
        else {
            HIPCHK(hipMemcpyAsync(c->bnd.d_pars.d(), c->bnd.h_pars.h(), nbytes, hipMemcpyHostToDevice, c->stream));
            dp = c->bnd.d_pars.d();
        }
    }
    ds = c->opt.zero_copy ? c->bnd.h_status.dv() : c->bnd.d_status.d();
    double *mine = c->gather.d.d() + (size_t)rank * n;
    if ((rc = launch_rows(c, dp, n, mine, ds, nullptr))) return rc;
    if ((rc = mbb_allgather_f64(c, mine, c->gather.d.d(), n))) return rc;
    HIPCHK(hipMemcpyAsync(c->gather.h.h(), c->gather.d.d(), total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (!c->opt.zero_copy)
        HIPCHK(hipMemcpyAsync(c->bnd.h_status.h(), c->bnd.d_status.d(), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if ((rc = wait_stream(c))) return rc;
    memcpy(all, c->gather.h.h(), total * sizeof(double));
    if (status) memcpy(status, c->bnd.h_status.h(), (size_t)n * sizeof(int32_t));
    return MBB_OK;
}

extern "C" int mbb_allgather_f64(mbb_ctx *c, const double *d_send, double *d_recv, int count)
{
    int rc = use(c);
    if (rc) return rc;
    if (!d_send || !d_recv || count < 0) return fail(MBB_ERR_ARG, "bad buffers");
    if (!c->comm) {
        if (c->nranks != 1) return fail(MBB_ERR_STATE, "communicator not initialised");
        if (d_send != d_recv)
            HIPCHK(hipMemcpyAsync(d_recv, d_send, (size_t)count * sizeof(double),
                                  hipMemcpyDeviceToDevice, c->stream));
        return MBB_OK;
    }
    int r = g_rccl.AllGather(d_send, d_recv, (size_t)count, 8 /* ncclFloat64 */, c->comm, c->stream);
    if (r != 0) return fail(MBB_ERR_RCCL, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "ncclAllGather failed");
    return MBB_OK;
}
