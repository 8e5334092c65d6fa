// vag_capi.hip -- C-ABI of the MI355X afterglow engine (include/vegasafterglow_amd.h).
// Host orchestration only: every number the library returns is produced by the gfx950 kernels in
// vag_grid_kernel.h / vag_kernels.h.  There is no CPU compute path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <shared_mutex>

#include "vag_ic_kernels.h"
#include "vag_kernels.h"
#include "vag_rs_kernels.h"
#include "vag_fit_rows.h"
#include "vag_grid_rows.h"
#include "vag_sky.h"
#include "vag_debug_math.h"
#include "vag_log_ndtr.h"
#include "vag_poisson.h"
#include "vag_index.h"
#include "vag_fit_kernels.h"
#include "vag_sampler.h"
#include "vag_tempering.h"
#include "vag_moves.h"
#include "vag_nested.h"
#include "vag_sampler_plan.h"
#include "vag_chain_stats.h"
#include "vag_predict.h"
#include "vag_fit_request.h"  // (host only: set_err, the scans, FitRequest)
#include "vag_flux_plan.h"    // (host only: the launch decisions of the flux stage)
#include "vag_stage_plan.h"   // (host only: the arithmetic of the model stages, the grouping by flags)

using namespace vag;

namespace {


// Developer / test hooks (VAG_* environment variables).  The process environment is read ONCE -- when the first hook is asked for, i.e.
// inside the first API call -- and again only by vag_reload_env_hooks(): no getenv on any call path afterwards (getenv races with
// setenv / putenv of other threads, and a thread pool drives one context from many threads).  A value's storage stays where
// it is until the next reload.
extern "C" char** environ;
struct EnvHooks {
    std::shared_mutex mu;
    std::map<std::string, std::string> kv;
    bool loaded = false;
    void load_locked() {
        kv.clear();
        for (char** e = environ; e && *e; ++e) {
            if (std::strncmp(*e, "VAG_", 4) != 0) continue;
            const char* eq = std::strchr(*e, '=');
            if (eq) kv.emplace(std::string(*e, eq - *e), std::string(eq + 1));
        }
        loaded = true;
    }
    const char* get(const char* name) {
        {
            std::shared_lock<std::shared_mutex> rd(mu);
            if (loaded) {
                auto it = kv.find(name);
                return it == kv.end() ? nullptr : it->second.c_str();
            }
        }
        std::unique_lock<std::shared_mutex> wr(mu);
        if (!loaded) load_locked();
        auto it = kv.find(name);
        return it == kv.end() ? nullptr : it->second.c_str();
    }
    void reload() {
        std::unique_lock<std::shared_mutex> wr(mu);
        load_locked();
    }
};
EnvHooks g_hooks;
inline const char* vag_hook(const char* name) { return g_hooks.get(name); }

#define HIPCHK(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return set_err(VAG_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// grow-only device buffer
// the grid kernel's three layouts (vag_common.h): 0 small (LDS, eight models per CU), 1 large (LDS, one per CU), 2 huge (scratch in HBM)
static int layout_theta(int level) { return level == 2 ? VAG_HUGE_THETA : (level == 1 ? VAG_MAX_THETA : VAG_GRID_THETA); }
static int layout_phi(int level) { return level == 2 ? VAG_HUGE_PHI : (level == 1 ? VAG_MAX_PHI : VAG_GRID_PHI); }
static int rowgeo_stride(int level) {  // doubles per model of the row-geometry records (vag_grid_kernel.h)
    return VAG_ROWGEO_HDR + 2 * layout_phi(level) + 4 * layout_theta(level);
}

// device memory this library holds in this process, all contexts (vag_device_bytes_in_use): every buffer in HBM is a DevBuf
static std::atomic<long long> g_device_bytes{0};
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) HIPCHK(hipFree(p));
        g_device_bytes -= (long long)cap;
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        HIPCHK(hipMalloc(&p, want));
        cap = want;
        g_device_bytes += (long long)cap;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        g_device_bytes -= (long long)cap;
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

struct HostBuf {  // pinned
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) HIPCHK(hipHostFree(p));
        p = nullptr;
        cap = 0;
        HIPCHK(hipHostMalloc(&p, bytes + bytes / 4 + 256, hipHostMallocDefault));
        cap = bytes + bytes / 4 + 256;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
};

// One spec block of the likelihood, resident on the device: the block goes up through its pinned staging copy only when its content
// hash or its size changes (a sampler loop calls with the same spec); a hit issues no HIP call.
struct ResidentBlock {
    HostBuf h;  // pinned staging copy
    DevBuf d;   // what the kernels read
    uint64_t hash = 0;
    size_t doubles = 0;  // of d
    bool valid = false;
    // The whole of it.  A hit returns.  A miss validates first: a refusal leaves the resident block as it was.  Then the stage (nothing
    // is resident, an earlier staging copy that may still be in flight is waited for, both buffers are sized), the fill of the pinned
    // buffer, and the commit.  tail: int32 the validation made; they ride behind the doubles in the pinned buffer and go to d_tail
    // (the visibility blocks).  A block of no doubles ends validated, not valid, nothing held.
    template <class Validate, class Fill>
    int upload(hipStream_t st, const BlockKey& key, Validate validate, Fill fill, const std::vector<int>* tail = nullptr, DevBuf* d_tail = nullptr) {
        const size_t n = key.doubles;
        if (valid && hash == key.hash && doubles == n) return VAG_OK;
        if (int rc = validate()) return rc;
        const size_t n_tail = tail ? tail->size() : 0;  // (the validation has made them)
        valid = false;
        if (n == 0) return VAG_OK;
        HIPCHK(hipStreamSynchronize(st));
        if (h.ensure(sizeof(double) * (n + (n_tail + 1) / 2)) || d.ensure(sizeof(double) * n)) return VAG_E_HIP;
        double* hp = h.as<double>();
        fill(hp);
        if (tail) {
            if (d_tail->ensure(sizeof(int) * n_tail)) return VAG_E_HIP;
            std::memcpy(hp + n, tail->data(), sizeof(int) * n_tail);
            HIPCHK(hipMemcpyAsync(d_tail->p, hp + n, sizeof(int) * n_tail, hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipMemcpyAsync(d.p, hp, sizeof(double) * n, hipMemcpyHostToDevice, st));
        hash = key.hash, doubles = n, valid = true;
        return VAG_OK;
    }
    void release() {
        h.release();
        d.release();
    }
};

enum { PS_DYNAMICS = 0, PS_SYN_ELECTRONS, PS_SYN_PHOTONS, PS_COOLING, PS_SYNC_FLUX, PS_IC_PHOTONS, PS_SSC_FLUX, PS_COUNT };

// prepares log2 arrays and the observer-time extrema on the device (single workgroup)
__global__ void vag_prep_kernel(const double* __restrict__ t, int nt, const double* __restrict__ nu, int nnu,
                                double* __restrict__ lg2_t, double* __restrict__ lg2_nu, double* __restrict__ tminmax) {
    __shared__ double s_min[256], s_max[256];
    double lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < nt; i += blockDim.x) {
        const double v = t[i];
        lo = fmin(lo, v);
        hi = fmax(hi, v);
        lg2_t[i] = log2(v * U_SEC);  // xt::log2(t_obs), observer.h:359
    }
    for (int i = threadIdx.x; i < nnu; i += blockDim.x) lg2_nu[i] = log2(nu[i] * U_HZ);
    s_min[threadIdx.x] = lo;
    s_max[threadIdx.x] = hi;
    __syncthreads();
    for (int off = blockDim.x / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + off]);
            s_max[threadIdx.x] = fmax(s_max[threadIdx.x], s_max[threadIdx.x + off]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tminmax[0] = s_min[0];
        tminmax[1] = s_max[0];
    }
}

}  // namespace

// ---- validation shared by host entry points; rules of pybind/pymodel.cpp:47-186, pymodel.h:205-260,613-649 ----
static bool finite_pos(double x) { return std::isfinite(x) && x > 0; }
static bool range_oi(double x, double lo, double hi) { return std::isfinite(x) && x > lo && x <= hi; }

static const char* validate_msg(const vag_model_params* p) {
    const double pi = 3.14159265358979323846;
    if (p->jet_type < 0 || p->jet_type > VAG_JET_POWERLAW_WING) return "unknown jet_type";
    if (p->jet_type == VAG_JET_MAGNETIZED_TOPHAT && !(std::isfinite(p->sigma0) && p->sigma0 >= 0))
        return "sigma0 must be finite and non-negative";
    if (p->medium_type < 0 || p->medium_type > VAG_MEDIUM_WIND) return "unknown medium_type";
    if (!range_oi(p->theta_c, 0.0, pi / 2)) return "theta_c must be in (0, pi/2]";
    if (p->jet_type != VAG_JET_POWERLAW_WING) {  // PowerLawWing has no core (pymodel.cpp:90-110)
        if (!finite_pos(p->E_iso)) return "E_iso must be positive and finite";
        if (!(std::isfinite(p->Gamma0) && p->Gamma0 > 1.0)) return "Gamma0 must be > 1";
    }
    if (!finite_pos(p->duration)) return "duration must be positive and finite";
    if (p->jet_type == VAG_JET_STEP_POWERLAW || p->jet_type == VAG_JET_POWERLAW_WING) {
        if (!finite_pos(p->E_iso_w)) return "E_iso_w must be positive and finite";
        if (!(std::isfinite(p->Gamma0_w) && p->Gamma0_w > 1.0)) return "Gamma0_w must be > 1";
    }
    if (p->jet_type == VAG_JET_POWERLAW || p->jet_type == VAG_JET_STEP_POWERLAW || p->jet_type == VAG_JET_POWERLAW_WING) {
        if (!finite_pos(p->k_e)) return "k_e must be positive and finite";
        if (!finite_pos(p->k_g)) return "k_g must be positive and finite";
    }
    if (p->jet_type == VAG_JET_TWO_COMPONENT) {
        if (!range_oi(p->theta_w, 0.0, pi / 2)) return "theta_w must be in (0, pi/2]";
        if (!(p->theta_w > p->theta_c)) return "theta_w (wing angle) must be greater than theta_c (core angle)";
        if (!finite_pos(p->E_iso_w)) return "E_iso_w must be positive and finite";
        if (!(std::isfinite(p->Gamma0_w) && p->Gamma0_w > 1.0)) return "Gamma0_w must be > 1";
    }
    if (p->medium_type == VAG_MEDIUM_ISM) {
        if (!(std::isfinite(p->n_ism) && p->n_ism >= 0)) return "n_ism must be non-negative and finite";
    } else {
        if (!finite_pos(p->A_star)) return "A_star must be positive and finite";
        if (!(std::isfinite(p->n_ism) && p->n_ism >= 0)) return "n_ism must be non-negative and finite";
        if (!(p->n0 > 0)) return "n0 must be > 0 (or +inf for no floor)";
        if (!finite_pos(p->k_m)) return "k_m must be positive and finite";
    }
    if (!finite_pos(p->lumi_dist)) return "lumi_dist must be positive and finite";
    if (!(std::isfinite(p->z) && p->z >= 0)) return "z must be non-negative and finite";
    if (!(std::isfinite(p->theta_obs) && p->theta_obs >= 0 && p->theta_obs <= pi)) return "theta_obs must be in [0, pi]";
    if (!range_oi(p->eps_e, 0.0, 1.0)) return "eps_e must be in (0, 1]";
    if (!range_oi(p->eps_B, 0.0, 1.0)) return "eps_B must be in (0, 1]";
    if (!range_oi(p->xi_e, 0.0, 1.0)) return "xi_e must be in (0, 1]";
    if (!(std::isfinite(p->p) && p->p > 1.0)) return "p must be > 1";
    if (!(std::isfinite(p->rtol) && p->rtol > 0 && p->rtol < 1)) return "rtol must be in (0, 1)";
    if (!finite_pos(p->phi_resol) || !finite_pos(p->theta_resol) || !finite_pos(p->t_resol))
        return "resolutions must be positive and finite";
    if (p->flags & VAG_FLAG_MAGNETAR) {  // PyMagnetar ctor, pymodel.h:45-49
        if (!finite_pos(p->mag_L0) || !finite_pos(p->mag_t0) || !finite_pos(p->mag_q)) return "magnetar L0, t0, q must be positive and finite";
        if (p->jet_type == VAG_JET_POWERLAW_WING || p->jet_type == VAG_JET_MAGNETIZED_TOPHAT) return "this jet type takes no magnetar";
    }
    if (p->flags & ~(VAG_FLAG_SSC | VAG_FLAG_KN | VAG_FLAG_RVS | VAG_FLAG_RVS_SSC | VAG_FLAG_RVS_KN | VAG_FLAG_SPREADING |
                     VAG_FLAG_MAGNETAR | VAG_FLAG_NON_AXISYMMETRIC))
        return "unknown bits set in flags";
    if (p->flags & VAG_FLAG_RVS) {  // rvs_rad is a Radiation too (pymodel.h:241-260)
        if (!range_oi(p->rvs_eps_e, 0.0, 1.0)) return "rvs eps_e must be in (0, 1]";
        if (!range_oi(p->rvs_eps_B, 0.0, 1.0)) return "rvs eps_B must be in (0, 1]";
        if (!range_oi(p->rvs_xi_e, 0.0, 1.0)) return "rvs xi_e must be in (0, 1]";
        if (!(std::isfinite(p->rvs_p) && p->rvs_p > 1.0)) return "rvs p must be > 1";
    }
    return nullptr;
}

// g(a) = log2(1 + 2^-a) interpolation table for sp_fast (vag_device.h): interval i is centred on the node a = i/SP_PER_UNIT
// and holds the degree-(SP_NCOEF-1) interpolant at Chebyshev nodes, converted to monomials in
// tau = a*SP_PER_UNIT - i in [-1/2, 1/2], all in long double.
// Returns the max abs error measured on a dense check grid.
static double build_softplus_table(std::vector<double>& tab) {
    const int n = SP_NCOEF, NI = SP_INTERVALS, per = SP_PER_UNIT;
    const long double PI = 3.141592653589793238462643383279502884L;
    tab.assign((size_t)NI * n, 0.0);
    long double T[SP_NCOEF][SP_NCOEF] = {};
    T[0][0] = 1;
    T[1][1] = 1;
    for (int k = 2; k < n; ++k)
        for (int q = 0; q < n; ++q) T[k][q] = (q > 0 ? 2 * T[k - 1][q - 1] : 0) - T[k - 2][q];
    for (int i = 0; i < NI; ++i) {
        const long double ac = (long double)i / per, h = 1.0L / per;
        long double f[SP_NCOEF], c[SP_NCOEF], mono[SP_NCOEF] = {};
        for (int j = 0; j < n; ++j) {
            const long double t = cosl(PI * (2 * j + 1) / (2 * n));
            f[j] = log2l(1 + exp2l(-(ac + h / 2 * t)));
        }
        for (int k = 0; k < n; ++k) {
            long double s = 0;
            for (int j = 0; j < n; ++j) s += f[j] * cosl(k * PI * (2 * j + 1) / (2 * n));
            c[k] = 2 * s / n;
        }
        c[0] /= 2;
        for (int k = 0; k < n; ++k)
            for (int q = 0; q < n; ++q) mono[q] += c[k] * T[k][q];
        long double sc = 1;
        for (int q = 0; q < n; ++q) {
            tab[(size_t)i * n + q] = (double)(mono[q] * sc);
            sc *= 2;
        }
    }
    double maxerr = 0;
    for (int i = 0; i < NI - 1; ++i)
        for (int s = 0; s <= 32; ++s) {
            const double a = (i + s / 32.0) / per;
            const double t = std::fma(a, (double)per, SP_MAGIC);  // same node selection as sp_fast
            const int idx = std::min((int)(t - SP_MAGIC), NI - 1);
            const double tau = std::fma(a, (double)per, -(t - SP_MAGIC));
            const double* c = &tab[(size_t)idx * n];
            double p = c[n - 1];
            for (int q = n - 2; q >= 0; --q) p = std::fma(p, tau, c[q]);
            const long double truth = log2l(1 + exp2l(-(long double)a));
            maxerr = std::max(maxerr, std::fabs((double)(p - truth)));
        }
    return maxerr;
}

// log2_tab (vag_device.h): entry i = {rc = double(1 / c_i), -log2(rc)} with c_i the centre of the i-th 1/64 slice of [1, 2).
// Returns the max error of the same arithmetic on the host relative to max(1, |log2 x|).
static double append_log2_table(std::vector<double>& tab) {
    for (int i = 0; i < LOG_TAB_N; ++i) {
        const double rc = (double)(1.0L / (1.0L + (i + 0.5L) / LOG_TAB_N));
        tab.push_back(rc);
        tab.push_back((double)(-log2l((long double)rc)));
    }
    const double* lt = tab.data() + tab.size() - LOG_TAB_DOUBLES;
    double maxerr = 0;
    for (int s = 0; s < 200000; ++s) {
        const double x = std::ldexp(1.0 + (s + 0.37) / 200000.0, (s % 41) - 20);
        int e;
        const double m = 2 * std::frexp(x, &e);  // [1, 2)
        e -= 1;
        const int idx = std::min((int)((m - 1) * LOG_TAB_N), LOG_TAB_N - 1);
        const double r = std::fma(m, lt[2 * idx], -1.0);
        double q = std::fma(1.0 / 7, r, -1.0 / 6);
        q = std::fma(q, r, 0.2);
        q = std::fma(q, r, -0.25);
        q = std::fma(q, r, 1.0 / 3);
        q = std::fma(q, r, -0.5);
        const double ln_m = std::fma(q * r, r, r);
        const double got = std::fma(ln_m, LOG2E, (double)e + lt[2 * idx + 1]);
        const long double want = log2l((long double)x);
        maxerr = std::max(maxerr, (double)(fabsl(got - want) / std::max(1.0L, fabsl(want))));
    }
    return maxerr;
}

// one answer of the occupancy query: resident workgroups per CU of a kernel at a block size and dynamic LDS (-1: the query failed)
struct Occupancy {
    const void* fn;
    int threads;
    size_t lds;
    int wg;
};
struct CoalesceRequest;
struct vag_ctx {
    int device = 0;
    // Every entry point that takes the context locks it for its duration (ApiLock): Model methods release the GIL and are called
    // from thread pools, one Model per thread (pybind.cpp:424-448, samplers.py:59-70), so the library serialises GPU access itself.
    std::recursive_mutex api_mutex;
    // Concurrent single-model calls gathered into batch calls (vag_*_coalesced, opt-in): see the coalescer below
    std::mutex co_mutex;
    std::condition_variable co_cv;  // the leader's: arrivals wake the leader alone (a waiting member sleeps on its own request's)
    std::vector<CoalesceRequest*> co_queue;
    bool co_leader = false;
    int co_max_batch = 64, co_wait_us = 50;
    long long co_calls = 0, co_batches = 0;  // requests served / batch calls issued (vag_ctx_coalesce_stats)
    // Likelihood calls evaluate the walkers in descending order of the cost the SAME batch position had in the previous call
    // (dispatch is in batch order: expensive walkers last leave the GPU draining, and neighbours of similar cost diverge less):
    // d_order[cur] maps evaluation slot -> walker; ln L, costs and counters come back in walker order.  A walker's ln L does
    // not depend on its slot, so the result is the same bits.
    DevBuf d_order[2], d_cost_f;  // d_cost_f: per-slot cost of the last batch (written with the batch plan by the grid kernel)
    int order_cur = 0, order_nb = 0;  // order_nb: batch size d_order[order_cur] was computed for (0: none)
    // sharded likelihood calls (vag_loglike_shard_dev): the gathered per-walker costs of the last finished call (what the next
    // deal ranks by), the current deal (walker of every (rank, slot)), this rank's gathered theta rows / ln L
    // The costs belong to a (fit data, batch size, world) triple: two fitters that alternate on one context must not rank each
    // other's walkers, so a few of them are kept (least recently used is replaced), keyed by the fit spec's content hash.
    struct ShardCosts {
        DevBuf cost;
        uint64_t hash = 0;
        int nb = 0, world = 0;
        bool valid = false;     // a call of this key has finished: `cost` holds its gathered costs
        int in_flight = 0;      // calls of this key that wait for their finish (the entry is not replaced meanwhile)
        unsigned long long used = 0;  // clock of the last use
    };
    // A call in flight (between its deal and its finish) owns ONE flight slot: the deal's table and the ticket that names it (ABI v13).
    // Until v12 the table hung on the key and a finish took "the oldest pending deal of this shape": two calls of equal shape that
    // finished in the opposite order to their deals applied each other's tables, and two calls of the SAME key could not both finish.
    struct ShardFlight {
        DevBuf table;           // walker of every (rank, slot); kept after the finish for inspection until the slot is dealt again
        uint64_t ticket = 0;    // the deal's clock value: unique per context, never 0
        int key = -1, nb = 0, world = 0;
        bool in_use = false;
        bool unticketed = false;  // opened by vag_loglike_shard_dev: a new deal of the same key replaces it (the v9 behaviour)
    };
    ShardCosts shard_costs[4];
    ShardFlight shard_flights[8];
    unsigned long long shard_clock = 0;
    int shard_last = -1;                    // key entry of the last finished call (vag_loglike_shard_state_dev reports its costs)
    int shard_last_dealt = -1;              // flight slot of the last deal (... and its table)
    DevBuf d_shard_theta, d_shard_ll;
    // device-resident batches whose models differ in their Radiation / shock flags: regrouped by flags (flux_dev_by_flags)
    bool mixed_flags_seen = false;  // the last grid pass stopped on such a batch
    DevBuf d_mix_flags, d_mix_perm, d_mix_params, d_mix_out;
    bool order_next = false, order_active = false;  // the next / the last model-stage run is in evaluation-slot order
    const int* last_order = nullptr;                // ... and the order it used
    int grid_large = 0;       // layout level of the grid kernel in use: 1 / 2 after a recent batch needed more than the small / large layout holds
    int grid_large_idle = 0;  // consecutive batches that would have fitted the small one
    DevBuf d_gridscratch;     // level 2: the grid kernel's scratch arrays, one GridSharedHuge per model
    std::vector<Occupancy> occ;     // occupancy-query results of the flux launches seen so far (wg_per_cu)
    DevBuf d_flux_order;            // [nb] deal order of a persistent vag_flux_grid_kernel launch (vag_flux_order_kernel)
    DevBuf d_partial2, d_ssc2;  // fused synchrotron + SSC flux pass: second partial-grid buffer / second scratch output
    DevBuf d_bandidx;  // [512 band index per point | 8 first point of each band] for the shared-node / row-per-lane series paths
    int h_bandbuf[512 + 8] = {};  // host mirror of d_bandidx (skips the upload while a fit keeps its data)
    int h_bands_n = -1;
    int pending_bands = 0;  // set by the host-pointer entry points that know the frequencies; consumed by the next series call
    DevBuf d_sptab, d_workcount, d_knlut, d_icy, d_cellq, d_band, d_icstatus, d_icunclamp, d_ssc;
    // SSC tables: a header per cell, the lattice plan between the plan and the spectrum kernel, and the pool of tables (each as long
    // as its own output lattice; offsets handed out by vag_ic_plan_kernel, d_icused counts the doubles in use)
    DevBuf d_ichdr, d_icplan, d_icpool, d_icused, d_icslow /* records of the cells on the spectrum kernel's slow path */;
    DevBuf d_skyterms, d_skyimg, d_skymom;  // sky images / moments (vag_sky.h): term list, a chunk's images, moments + outside
    DevBuf d_skypol, d_skystokes;  // polarization (vag_sky.h): a chunk's row-block partials, the models' spec + Stokes sums + outside
    DevBuf d_skyvis, d_skyuv;  // visibilities (vag_sky.h): a chunk's row-block partials + combined values, a chunk's baselines
    DevBuf d_skycen, d_skycmom;  // exact centroids (vag_sky.h): row-block partials, moments
    DevBuf d_visblk, d_vispart;  // visibility groups of the likelihood (their data: vis below): their 64-visibility blocks, chi^2 partials
    DevBuf d_sampler_prop, d_sampler_fresh, d_sampler_aux;  // the device sampler's run entries (sampler_run), one set for the three moves, as large as the largest run so far: a half-step's proposals [nb][ndim], their ln p or ln L [nb], their Hastings factor or ln prior [nb]
    DevBuf d_nested_rank;  // nested sampling's run entry (vag_nested_run_dev): L* [1], then the slots by rank, int32 [N]
    DevBuf d_chain_stats;  // chain autocorrelation (vag_chain_autocorr_dev): the means [S], the lag sums [L + 1][S], the pooled sums [L + 1][D]
    DevBuf d_predict;  // posterior-predictive bands (vag_column_quantiles_dev, vag_predict_bands_dev): the draws' A_V [S] and, where the caller keeps none, their fluxes [S][M]; behind them int32: the engine's verdict [S], the validity [S]
    DevBuf d_polspec, d_polstokes;  // polarization groups of the likelihood (their data: pol below): the walkers' spec + its flag, jet-frame I, Q, U
    DevBuf d_icneed;  // [cells] bytes: 1 = some (theta, phi) row's observation window touches the cell (vag_ic_band_kernel)
    bool count_work = false;
    bool ic_all_cells = false;    // this request's SSC tables are built for every cell (the lazy selection was caught with a hole, see check_ic_status)
    int batch_flags = 0;  // VAG_FLAG_* shared by every model of the current batch
    // reverse shock (VAG_FLAG_RVS): its own shock / electron / photon arrays and radiation parameters.  The radiation and
    // flux passes always read d_shock, d_cellpar, ...; select_emitter() swaps the reverse shock's buffers in and out.
    DevBuf d_shock_r, d_cellpar_r, d_celldet_r, d_icy_r, d_cellq_r, d_params_rvs, d_inj, d_comp;
    DevBuf d_fail;     // int[16], reset per batch by the grid kernel: ODE rows per status ([1] step underflow, [2] step cap, [3] stalled); three 64-bit tallies at
                       // [8..13] (vag_ctx_count_work: right-hand sides, live lanes over the attempts, lane slots of the attempts).  (The row queue of the refill kernel is not here: it lives in d_dynrec.)
    DevBuf d_dynrec;   // [rows][DYN_ROWREC] start records of vag_dynamics_refill_kernel (vag_dyn_prep_kernel)
    int dyn_refill_wg_per_cu = 0;  // resident wavefronts of that kernel per CU (occupancy query, once)
    DevBuf d_cellgeo;  // spreading jets (VAG_FLAG_SPREADING): per-cell cos/sin(theta), log2|dcos|, shared by both shocks
    int cur_emitter = 0;                            // 0 forward, 1 reverse
    bool cur_ssc = false;                           // SSC switch of the selected emitter
    const vag_model_params* cur_params = nullptr;   // parameters its radiation / flux kernels read
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    hipEvent_t ev[8] = {};
    hipEvent_t ev_handoff = nullptr;  // orders the context's buffers across a change of stream (vag_ctx_set_stream)
    bool handoff_ready = false;       // ev_handoff marks the tail of the work queued on the current (caller-owned) stream
    bool handoff_dirty = false;       // a compute call has queued work since the event was last recorded (ApiLock records it on the way out)
    // inputs
    DevBuf d_params, d_t, d_nu, d_lg2t, d_lg2nu, d_tminmax, d_bandw, d_out;
    // grid results
    DevBuf d_meta, d_phi, d_theta, d_rep_of, d_rep_start, d_tdec, d_geo_th, d_geo_ph;
    HostBuf h_meta, h_off, h_plan;
    DevBuf d_plan;                // VagDevPlan of the current batch (vag_plan_kernel)
    DevBuf d_chunk;               // staging of chunked requests
    DevBuf d_icwork;              // work tallies of the SSC tables (vag_ic_plan_kernel, vag_ctx_count_work)
    VagDevPlan hint{};            // the last plan the host read back: sizes the next call of the same batch size in advance
    int hint_nb = 0;
    bool hint_valid = false;
    bool spec_pending = false;    // the current call was planned from the hint and has not been verified yet
    VagDevPlan* d_hplan = nullptr;  // device address of h_plan
    int plan_seq = 0;
    int layout_large = 0;  // vag_grid_kernel's layout level of the batch at hand
    DevBuf d_rowgeo;            // row-geometry records for the flux grid kernel, written by the grid kernel
    bool plan_counter_ready = false;
    int n_cus = 256;              // compute units of the device (persistent launches size themselves by it)
    // named-stage profiler (vag_ctx_profile): spans of (stage id, begin event, end event) recorded during a call
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;
    struct ProfSpan { int id, e0, e1; };
    std::vector<ProfSpan> prof_spans;
    int prof_used = 0;
    int spec_cap_k = 0;
    int spec_margin_k = 2;        // lattice nodes of head room in a planned-ahead call; grows when a call had to be repeated
    bool meta_on_host = false;    // h_meta holds the current batch's grid results (copied on demand)
    // compact per-row / per-cell storage
    DevBuf d_row_off, d_cell_off, d_shock, d_cellpar, d_row_status, d_celldet, d_partial;
    DevBuf d_theta_in, d_valid, d_series_flux, d_chi2, d_bandobs, d_fitstat;
    // the likelihood's spec blocks, one ResidentBlock each (layouts, scans and fills: vag_fit_request.h; uploads: upload_blocks)
    ResidentBlock fit;     // the observation arrays, the slot map and the priors of the vag_fit_spec, see FitLayout
    ResidentBlock sky;     // centroid groups (vag_loglike_sky_batch): per group [nu | six arrays], see SkyLayout
    ResidentBlock vis;     // visibility groups (vag_loglike_vis_batch); their int32 blocks are d_visblk, their places vis_layout
    ResidentBlock pol;     // polarization groups (vag_loglike_pol_batch): per group [nu | six arrays], see PolLayout
    ResidentBlock lim;     // upper-limit rows (vag_loglike_lim_batch): per block [limit | sigma | kind], see LimLayout
    ResidentBlock noise;   // noise groups (vag_loglike_noise_batch): [sys_fixed 8 | calib 8] then per pass the rows' group ids, see NoiseLayout
    ResidentBlock counts;  // counts groups (vag_loglike_counts_batch): per group [t_sample | N | B | a | w | idx], see CountsLayout
    ResidentBlock index;   // spectral-index groups (vag_loglike_index_batch): per group [t | nu | s | sigma | w | c], see IndexLayout
    ResidentBlock fold;    // fold groups (vag_loglike_fold_batch): per group the block FoldLayout describes
    ResidentBlock tmpl;    // additive templates (vag_loglike_tmpl_batch): [amp_fixed 8] then per touched pass its [n_templates][n] values, see TmplLayout
    ResidentBlock cov;     // correlated groups (vag_loglike_cov_batch): per group [t | nu | ln_flux | ext | Wt], see CovLayout
    ResidentBlock robust;  // outlier groups (vag_loglike_robust_batch): [frac_fixed 8 | scale_fixed 8 | shift_fixed 8], see RobustLayout
    std::vector<VisLayout> vis_layout;  // of the resident visibility groups: made by the miss that made them resident
    bool fit_stats_pending = false;  // d_fitstat of the last likelihood call not read back yet
    bool ic_need_reset = true;       // first SSC table build of a pass clears d_icstatus
    bool ic_soft_fail = false;       // likelihood calls: SSC table failures invalidate the walker instead of raising
    bool ic_slow_unread = false;     // the last table build did not wait for its counters: vag_last_plan reads the slow path's from HBM
    // plan of the last grid pass
    int nb = 0, n_rows = 0, max_k = 0, max_pairs = 0;
    int ppb_pin = 0;  // > 0: the (theta, phi) pairs per flux workgroup of the next grid / band request, whatever the batch holds (choose_pairs_per_block)
    long long n_cells = 0, total_pairs = 0, eat_cells = 0;
    int n_ok = 0;
    vag_plan plan{};
    vag_stage_times times{};
};

// One profiled stage: begin / end events on the context stream while the profiler is on (vag_ctx_profile)
struct StageScope {
    vag_ctx* c;
    int span = -1;
    StageScope(vag_ctx* ctx, int id) : c(ctx) {
        if (!c->prof_on) return;
        if (c->prof_used + 2 > (int)c->prof_ev.size()) {
            for (int i = 0; i < 16; ++i) {
                hipEvent_t e;
                if (hipEventCreate(&e) != hipSuccess) return;
                c->prof_ev.push_back(e);
            }
        }
        span = (int)c->prof_spans.size();
        c->prof_spans.push_back({id, c->prof_used, c->prof_used + 1});
        (void)hipEventRecord(c->prof_ev[c->prof_used], c->stream);
        c->prof_used += 2;
    }
    ~StageScope() {
        if (span >= 0) (void)hipEventRecord(c->prof_ev[c->prof_spans[span].e1], c->stream);
    }
};

// A call mode: a context field that holds `v` for a scope and its earlier value after it, whichever way the scope is left
// (ppb_pin, pending_bands, ic_soft_fail, ic_all_cells).
template <class T>
struct CallMode {
    T& field;
    const T before;
    CallMode(T& f, T v) : field(f), before(f) { field = v; }
    ~CallMode() { field = before; }
    CallMode(const CallMode&) = delete;
};

extern "C" {

const char* vag_last_error(void) { return g_err.c_str(); }
struct ApiLock {  // (a null context is rejected by the entry point itself)
    std::recursive_mutex* m;
    vag_ctx* ctx;
    explicit ApiLock(vag_ctx* c);
    ~ApiLock();
    ApiLock(const ApiLock&) = delete;
};
const char* vag_version(void) { return "vegasafterglow_amd 0.1 (gfx950)"; }
void vag_reload_env_hooks(void) { g_hooks.reload(); }
int vag_abi_version(void) { return VAG_ABI_VERSION; }

void vag_params_default(vag_model_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->jet_type = VAG_JET_TOPHAT;
    p->medium_type = VAG_MEDIUM_ISM;
    p->theta_c = 0.1;
    p->E_iso = 1e52;
    p->Gamma0 = 300;
    p->k_e = 2;
    p->k_g = 2;
    p->theta_w = 3.14159265358979323846 / 2;
    p->E_iso_w = 1e52;
    p->Gamma0_w = 300;
    p->duration = 1;
    p->n_ism = 1;
    p->A_star = 0;
    p->n0 = INFINITY;
    p->k_m = 2;
    p->lumi_dist = 1e28;
    p->z = 0;
    p->theta_obs = 0;
    p->eps_e = 0.1;
    p->eps_B = 0.01;
    p->p = 2.3;
    p->xi_e = 1;
    p->phi_resol = 0.06;
    p->theta_resol = 0.15;
    p->t_resol = 6;
    p->rtol = 1e-6;
    p->radiative_fireball = 1;
}

int vag_params_validate(const vag_model_params* p) {
    if (!p) return set_err(VAG_E_INVALID, "null model");
    const char* msg = validate_msg(p);
    return msg ? set_err(VAG_E_INVALID, "%s", msg) : VAG_OK;
}

int vag_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

long long vag_device_bytes_in_use(void) { return g_device_bytes.load(); }

void vag_get_limits(vag_limits* out) {
    out->max_theta = VAG_HUGE_THETA;
    out->max_phi = VAG_HUGE_PHI;
    out->max_time = VAG_MAX_TIME;
    out->max_nu = VAG_MAX_NU;
}

}  // extern "C"

// streams, events, kernel attributes and the request-independent tables of a fresh context
static int ctx_init(vag_ctx* c) {
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    for (auto& e : c->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreateWithFlags(&c->ev_handoff, hipEventDisableTiming));
    HIPCHK(hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    // allow the flux kernels the full 160 KiB LDS of a gfx950 CU
    for (const void* fn : {reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<true, FLUX_SYN>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN_IC>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SSC>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN, false, 256>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN_IC, false, 256>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SSC, false, 256>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN, true>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SYN_IC, true>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_SSC, true>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_FUSED>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_FUSED, false, 256>),
                           reinterpret_cast<const void*>(vag_flux_grid_kernel<false, FLUX_FUSED, true>),
                           reinterpret_cast<const void*>(vag_flux_grid_split_kernel),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN, true>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN_IC, true>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SSC, true>)})
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    // the quantile kernel's sorted tile: 16 + VAG_PREDICT_LDS_BYTES at most (vag_predict.h)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(vag_predict_quantile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    {   // Klein-Nishina cross-section table (ComptonSigmaLUT, src/radiation/inverse-compton.cpp:285-300): request-independent
        std::vector<double> lut(2 * KN_LUT_N);
        const double step = (KN_LG2_XMAX - KN_LG2_XMIN) / (double)(KN_LUT_N - 1);
        for (int i = 0; i < KN_LUT_N; ++i) {
            const double x = std::exp2(KN_LG2_XMIN + step * (double)i);
            double ratio;
            if (x < 1e-2) {
                ratio = 1 - 2 * x;
            } else if (x > 1e2) {
                ratio = 3. / 8 * (std::log(2 * x) + 0.5) / x;
            } else {
                const double l = std::log1p(2.0 * x), invx = 1.0 / x, invx2 = invx * invx;
                const double invt1 = 1.0 / (1.0 + 2.0 * x), invt1_2 = invt1 * invt1;
                ratio = 0.75 * ((1.0 + x) * invx2 * invx * (2.0 * x * (1.0 + x) * invt1 - l) + 0.5 * l * invx -
                                (1.0 + 3.0 * x) * invt1_2);
            }
            lut[i] = ratio;
            lut[KN_LUT_N + i] = std::log2(ratio);
        }
        if (c->d_knlut.ensure(sizeof(double) * lut.size())) return VAG_E_HIP;
        HIPCHK(hipMemcpy(c->d_knlut.p, lut.data(), sizeof(double) * lut.size(), hipMemcpyHostToDevice));
    }
    for (const void* fn : {reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN_IC>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SSC>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN, false, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN_IC, false, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SSC, false, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN, true, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN_IC, true, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SSC, true, 1>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN, false, SERIES_MAX_SLOTS, true>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN_IC, false, SERIES_MAX_SLOTS, true>),
                           reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SSC, false, SERIES_MAX_SLOTS, true>)})
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    {
        std::vector<double> tab;
        const double err = build_softplus_table(tab);
        if (!(err < 5e-14)) return set_err(VAG_E_HIP, "softplus table accuracy check failed: %.3e", err);
        const double lerr = append_log2_table(tab);  // [SP_TABLE_DOUBLES, SP_LDS_DOUBLES): log2_tab's {1/c, -log2(1/c)} pairs
        if (!(lerr < 4e-16)) return set_err(VAG_E_HIP, "log2 table accuracy check failed: %.3e", lerr);
        if (c->d_sptab.ensure(sizeof(double) * tab.size())) return VAG_E_HIP;
        HIPCHK(hipMemcpy(c->d_sptab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    }
    return VAG_OK;
}

extern "C" {

ApiLock::ApiLock(vag_ctx* c) : m(c ? &c->api_mutex : nullptr), ctx(c) {
    if (m) m->lock();
}
// EVERY entry point leaves the hand-off event at the tail of a caller-owned stream, whichever way it returns (only the
// device-pointer forms did, so a host-buffer call that failed with kernels still queued left `handoff_ready` stale and the next
// vag_ctx_set_stream ordered the new stream behind an older event -- scratch buffers could be reused while the old stream wrote them).
// (Only on the way out of a call that queued work -- `handoff_dirty`, set where a call's model stage starts: the getters may be called
// after the caller destroyed its stream and must not touch it.)
ApiLock::~ApiLock() {
    if (ctx && ctx->handoff_dirty && ctx->stream != nullptr && ctx->stream != ctx->own_stream && ctx->ev_handoff) {
        ctx->handoff_ready = hipEventRecord(ctx->ev_handoff, ctx->stream) == hipSuccess;
        ctx->handoff_dirty = false;
    }
    if (m) m->unlock();
}

int vag_ctx_create(int device, vag_ctx** out) {
    if (!out) return set_err(VAG_E_INVALID, "null output pointer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(VAG_E_NO_DEVICE, "no HIP device available: the engine has no CPU path");
    if (device < 0 || device >= n) return set_err(VAG_E_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIPCHK(hipSetDevice(device));
    vag_ctx* c = new vag_ctx();
    c->device = device;
    const int rc = ctx_init(c);
    if (rc) {  // nothing half-built survives a failed creation
        vag_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return VAG_OK;
}

void vag_ctx_destroy(vag_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf* b : {&c->d_flux_order, &c->d_partial2, &c->d_ssc2, &c->d_bandidx, &c->d_sptab, &c->d_workcount, &c->d_knlut, &c->d_icy, &c->d_cellq, &c->d_band, &c->d_ichdr, &c->d_icplan, &c->d_icpool, &c->d_icused, &c->d_icslow,
                      &c->d_icstatus, &c->d_icunclamp, &c->d_ssc, &c->d_shock_r, &c->d_cellpar_r, &c->d_celldet_r, &c->d_icy_r,
                      &c->d_cellq_r, &c->d_params_rvs, &c->d_inj, &c->d_comp, &c->d_cellgeo, &c->d_fail, &c->d_dynrec, &c->d_gridscratch, &c->d_chi2, &c->d_bandobs, &c->d_params, &c->d_t, &c->d_nu, &c->d_lg2t, &c->d_lg2nu, &c->d_tminmax, &c->d_bandw, &c->d_out,
                      &c->d_meta, &c->d_phi, &c->d_theta, &c->d_rep_of, &c->d_rep_start, &c->d_tdec, &c->d_geo_th, &c->d_geo_ph, &c->d_row_off,
                      &c->d_cell_off, &c->d_shock, &c->d_cellpar, &c->d_row_status, &c->d_celldet, &c->d_partial,
                      &c->d_theta_in, &c->d_valid, &c->d_series_flux})
        b->release();
    c->h_meta.release();
    c->h_off.release();
    c->h_plan.release();
    c->d_plan.release();
    c->d_chunk.release();
    c->d_icwork.release();
    for (ResidentBlock* b : {&c->fit, &c->sky, &c->vis, &c->pol, &c->lim, &c->noise, &c->counts, &c->index, &c->fold, &c->tmpl, &c->cov, &c->robust}) b->release();
    c->d_fitstat.release();
    for (DevBuf* b : {&c->d_mix_flags, &c->d_mix_perm, &c->d_mix_params, &c->d_mix_out, &c->shard_costs[0].cost, &c->shard_costs[1].cost, &c->shard_costs[2].cost, &c->shard_costs[3].cost, &c->shard_flights[0].table, &c->shard_flights[1].table, &c->shard_flights[2].table, &c->shard_flights[3].table, &c->shard_flights[4].table, &c->shard_flights[5].table, &c->shard_flights[6].table, &c->shard_flights[7].table, &c->d_shard_theta, &c->d_shard_ll, &c->d_order[0], &c->d_order[1], &c->d_cost_f, &c->d_rowgeo, &c->d_icneed, &c->d_skyterms, &c->d_skyimg, &c->d_skymom, &c->d_skyvis, &c->d_skyuv, &c->d_skypol, &c->d_skystokes, &c->d_skycen, &c->d_skycmom, &c->d_visblk, &c->d_vispart, &c->d_polspec, &c->d_polstokes, &c->d_sampler_prop, &c->d_sampler_fresh, &c->d_sampler_aux, &c->d_nested_rank, &c->d_chain_stats, &c->d_predict})
        b->release();
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->ev_handoff) (void)hipEventDestroy(c->ev_handoff);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int vag_ctx_set_stream(vag_ctx* c, void* s) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    hipStream_t next;
    if (s == VAG_STREAM_LEGACY_DEFAULT)
        next = nullptr;  // the legacy default stream
    else
        next = s ? reinterpret_cast<hipStream_t>(s) : c->own_stream;
    if (next != c->stream) {
        // The context's scratch buffers (parameters, grid results, shock arrays, deal tables ...) are reused by every call, so
        // work queued on the stream the context leaves must be ordered before anything the next stream does with them: an event
        // at the tail of the old stream, waited for by the new one.  No host synchronisation.
        (void)hipSetDevice(c->device);
        const bool foreign = c->stream != nullptr && c->stream != c->own_stream;
        if (!foreign) {  // the context's own stream / the legacy default stream: always alive, the event is recorded here
            if (hipEventRecord(c->ev_handoff, c->stream) != hipSuccess) return set_err(VAG_E_HIP, "vag_ctx_set_stream: event record failed");
            c->handoff_ready = true;
        }
        // a caller-owned stream may have been destroyed since its last call (legal: nothing can be in flight on it then), so it is
        // never touched here: every device-resident entry point records the event at its own end, while the stream is known to be
        // alive (HandoffScope), and the host-buffer entry points end with a synchronisation
        if (c->handoff_ready && hipStreamWaitEvent(next, c->ev_handoff, 0) != hipSuccess)
            return set_err(VAG_E_HIP, "vag_ctx_set_stream: the new stream cannot wait for the work queued on the old one");
        c->handoff_ready = false;
        c->stream = next;
    }
    return VAG_OK;
}

// At the end of an entry point that leaves work in flight on a caller-owned stream: the hand-off event of vag_ctx_set_stream
struct HandoffScope {
    vag_ctx* c;
    explicit HandoffScope(vag_ctx* ctx) : c(ctx) {}
    ~HandoffScope() {
        if (c && c->stream != nullptr && c->stream != c->own_stream)
            c->handoff_ready = hipEventRecord(c->ev_handoff, c->stream) == hipSuccess;
    }
};

int vag_ctx_get_stream(vag_ctx* c, void** out) {
    ApiLock api_lock(c);
    if (!c || !out) return set_err(VAG_E_INVALID, "null context or pointer");
    if (c->stream == c->own_stream)
        *out = nullptr;
    else
        *out = c->stream ? reinterpret_cast<void*>(c->stream) : VAG_STREAM_LEGACY_DEFAULT;
    return VAG_OK;
}

int vag_ctx_count_work(vag_ctx* c, int enable) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    c->count_work = enable != 0;
    return VAG_OK;
}

static int read_row_failures(vag_ctx* c) {
    int f[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (c->d_fail.p && c->n_rows > 0) {
        HIPCHK(hipMemcpyAsync(f, c->d_fail.p, sizeof f, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    c->plan.n_rows_failed = f[1];
    c->plan.n_rows_gave_up = f[2] + f[3];
    {   // 64-bit tallies (vag_ctx_count_work; ADVICE r05: the int32 counter wrapped beyond ~3 M rows)
        unsigned long long t64[3];
        std::memcpy(t64, f + 8, sizeof t64);
        c->plan.ode_rhs = (long long)t64[0];
        c->plan.ode_lane_attempts = (long long)t64[1];
        c->plan.ode_lane_slots = (long long)t64[2];
    }
    if (c->fit_stats_pending && c->d_fitstat.p) {  // the last likelihood call's tallies over ALL of its passes
        int fs[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(fs, c->d_fitstat.p, sizeof fs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->plan.n_walkers_rejected = fs[0];
        c->plan.n_walkers_ssc_failed = fs[1];
        c->fit_stats_pending = false;
    }
    if (c->ic_slow_unread && c->d_icused.p) {  // a likelihood call's LAST table build (the builds before it reused the counters)
        unsigned long long n = 0;
        HIPCHK(hipMemcpyAsync(&n, c->d_icused.as<unsigned long long>() + 3, sizeof n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->plan.n_ssc_slow_cells += (long long)n;
        c->ic_slow_unread = false;
    }
    return VAG_OK;
}

int vag_last_plan(vag_ctx* c, vag_plan* out) {
    ApiLock api_lock(c);
    if (!c || !out) return set_err(VAG_E_INVALID, "null context or output");
    const int rc = read_row_failures(c);
    *out = c->plan;
    return rc;
}

int vag_ctx_synchronize(vag_ctx* c) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    HIPCHK(hipStreamSynchronize(c->stream));
    return VAG_OK;
}

int vag_ctx_profile(vag_ctx* c, int enable) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    c->prof_on = enable != 0;
    return VAG_OK;
}

int vag_last_profile(vag_ctx* c, vag_profile* out) {
    ApiLock api_lock(c);
    if (!c || !out) return set_err(VAG_E_INVALID, "null context or output");
    HIPCHK(hipStreamSynchronize(c->stream));
    double acc[PS_COUNT] = {0};
    float first = 0, last = 0;
    for (size_t i = 0; i < c->prof_spans.size(); ++i) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, c->prof_ev[c->prof_spans[i].e0], c->prof_ev[c->prof_spans[i].e1]));
        acc[c->prof_spans[i].id] += ms;
        float to_end = 0;
        HIPCHK(hipEventElapsedTime(&to_end, c->prof_ev[c->prof_spans[0].e0], c->prof_ev[c->prof_spans[i].e1]));
        last = std::max(last, to_end);
    }
    (void)first;
    *out = vag_profile{acc[PS_DYNAMICS], 0.0, acc[PS_SYN_ELECTRONS], acc[PS_SYN_PHOTONS], acc[PS_COOLING], acc[PS_SYNC_FLUX],
                       acc[PS_IC_PHOTONS], acc[PS_SSC_FLUX], (double)last};
    return VAG_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// pipeline stages (host orchestration)
// ------------------------------------------------------------------------------------------------
namespace {

// Swap the reverse shock's arrays into (e = 1) or out of (e = 0) the slots every radiation / flux pass reads, and
// point the passes at the matching radiation parameters (single_shock_emission is the same code for both shocks,
// pybind/pymodel.h:877-920).
void select_emitter(vag_ctx* c, int e, const vag_model_params* d_params) {
    if (e != c->cur_emitter) {
        std::swap(c->d_shock, c->d_shock_r);
        std::swap(c->d_cellpar, c->d_cellpar_r);
        std::swap(c->d_celldet, c->d_celldet_r);
        std::swap(c->d_icy, c->d_icy_r);
        std::swap(c->d_cellq, c->d_cellq_r);
        c->cur_emitter = e;
    }
    if (e == 0) {
        c->cur_params = d_params;
        c->cur_ssc = (c->batch_flags & VAG_FLAG_SSC) != 0;
    } else {
        c->cur_params = c->d_params_rvs.as<vag_model_params>();
        c->cur_ssc = (c->batch_flags & VAG_FLAG_RVS_SSC) != 0;
    }
}

// Stage 3 for the selected emitter: electrons + photons per cell (generate_syn_electrons / generate_syn_photons),
// then apply_ic_cooling (pybind/pymodel.h:567-577) when its Radiation has ssc.
int run_radiation(vag_ctx* c, const vag_model_params* d_rad_params, int nb, const int* d_inj, bool ssc, bool want_details,
                  bool raw_shock = false) {
    hipStream_t st = c->stream;
    const long long cells = c->n_cells;
    const int rows = c->n_rows;
    if (c->d_cellpar.ensure(sizeof(double) * (size_t)cells * VAG_NPAR)) return VAG_E_HIP;
    if (ssc) want_details = true;  // the cooling pass works on the electron arrays
    if (want_details && c->d_celldet.ensure(sizeof(double) * (size_t)cells * VAG_NDET)) return VAG_E_HIP;
    Layout lay{c->d_row_off.as<int>(), c->d_cell_off.as<long long>()};
    {
        StageScope ps(c, PS_SYN_ELECTRONS);
        hipLaunchKernelGGL(vag_cells_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, d_rad_params, nb,
                           c->d_meta.as<VagGridMeta>(), lay, c->d_shock.as<double>(), cells, c->d_cellpar.as<double>(),
                           want_details ? c->d_celldet.as<double>() : nullptr, d_inj, raw_shock ? c->d_shock.as<double>() : nullptr,
                           want_details || vag_hook("VAG_CELLS_WRITE_BACK") != nullptr);
    }
    HIPCHK(hipGetLastError());
    if (ssc) {  // cool the electrons row by row, then rebuild the photons
        if (c->d_icy.ensure(sizeof(double) * (size_t)cells * VAG_NICY)) return VAG_E_HIP;
        if (c->d_cellq.ensure(sizeof(double) * (size_t)cells * VAG_NQ)) return VAG_E_HIP;
        {
            StageScope ps(c, PS_COOLING);
            hipLaunchKernelGGL(vag_ic_cooling_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, d_rad_params, nb,
                               c->d_meta.as<VagGridMeta>(), lay, rows, c->d_shock.as<double>(), cells, c->d_celldet.as<double>(),
                               d_inj);
        }
        HIPCHK(hipGetLastError());
        {
            StageScope ps(c, PS_SYN_PHOTONS);
            hipLaunchKernelGGL(vag_photons_ic_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, d_rad_params, nb,
                               c->d_meta.as<VagGridMeta>(), lay, c->d_shock.as<double>(), cells, c->d_celldet.as<double>(),
                               c->d_icy.as<double>(), c->d_cellpar.as<double>(), c->d_cellq.as<double>(), d_inj);
        }
        HIPCHK(hipGetLastError());
    }
    return VAG_OK;
}

// Wait until the grid kernel of the current call has published its batch summary in pinned host memory (plan_scan_wave writes
// the sequence number last).  A spin on host memory: no copy, no stream synchronisation, the queue behind the grid kernel keeps
// running.  Falls back to a stream synchronisation if the number does not arrive (a failed launch).
int wait_plan(vag_ctx* c) {
    volatile VagDevPlan* hp = c->h_plan.as<VagDevPlan>();
    const auto t0 = std::chrono::steady_clock::now();
    for (long long spins = 0; hp->seq != c->plan_seq; ++spins) {
        __builtin_ia32_pause();
        if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            HIPCHK(hipStreamSynchronize(c->stream));
            if (hp->seq != c->plan_seq) return set_err(VAG_E_HIP, "the grid stage did not publish its batch summary");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return VAG_OK;
}

// a hook as the decisions of vag_flux_plan.h / vag_stage_plan.h take it: std::atoi of the variable, HOOK_UNSET where it is not set
static int hook_int(const char* name) {
    const char* e = vag_hook(name);
    return e ? std::max(std::atoi(e), HOOK_UNSET + 1) : HOOK_UNSET;
}
static DynHooks dyn_hooks() {  // (DynHooks' members in their order)
    return {hook_int("VAG_DYN_GENERAL"), hook_int("VAG_DYN_REFILL"), hook_int("VAG_DYN_REFILL_MIN"), hook_int("VAG_DYN_REFILL_WGS"),
            hook_int("VAG_PAIR_RPW"), hook_int("VAG_DYN_RPW")};
}

// Stage 1-3: adaptive grid -> blast-wave dynamics -> per-cell radiation, for nb models whose
// parameters are already in HBM.  d_tminmax holds the observer-time extrema [s].
// may_plan: the caller ends with finish_speculation() and repeats the call where that says so
int run_model_stages(vag_ctx* c, const vag_model_params* d_params, int nb, bool want_details, bool may_plan = false) {
    c->handoff_dirty = true;  // work is about to be queued on the context stream (ApiLock::~ApiLock)
    c->order_active = c->order_next;  // only a likelihood call that permuted its walkers sets order_next (vag_ctx::d_order)
    c->order_next = false;
    hipStream_t st = c->stream;
    if (c->d_meta.ensure(sizeof(VagGridMeta) * nb)) return VAG_E_HIP;
    if (c->d_cost_f.ensure(sizeof(float) * nb)) return VAG_E_HIP;
    // per-model angular arrays at the stride of the layout the grid kernel runs with (VagGridMeta::th_stride / ph_stride): 17 KB per
    // model for default-resolution batches (256 theta / 208 phi slots), 140 KB when a batch needed the large layout
    auto ensure_angular = [&](int large) -> bool {
        const size_t ts = layout_theta(large), ps = layout_phi(large);
        if (large == 2 && c->d_gridscratch.ensure(sizeof(GridSharedHuge) * (size_t)nb)) return true;
        return c->d_phi.ensure(sizeof(double) * (size_t)nb * ps) || c->d_theta.ensure(sizeof(double) * (size_t)nb * ts) ||
               c->d_tdec.ensure(sizeof(double) * (size_t)nb * 3 * ts) || c->d_geo_th.ensure(sizeof(double) * (size_t)nb * 3 * ts) ||
               c->d_geo_ph.ensure(sizeof(double) * (size_t)nb * 2 * ps) || c->d_rep_of.ensure(sizeof(int) * (size_t)nb * ts) ||
               c->d_rep_start.ensure(sizeof(int) * (size_t)nb * ts) || c->d_rowgeo.ensure(sizeof(double) * (size_t)nb * rowgeo_stride(large));
    };
    if (const char* e = vag_hook("VAG_GRID_FORCE_LARGE"))  // test hook: the large (1) / huge (2) layout for batches that fit the small one
        c->grid_large = std::max(c->grid_large, std::atoi(e) == 2 ? 2 : 1), c->grid_large_idle = 0;
    if (ensure_angular(c->grid_large)) return VAG_E_HIP;
    if (c->d_row_off.ensure(sizeof(int) * 2 * (size_t)(nb + 1))) return VAG_E_HIP;  // [nb + 1] row offsets, [nb + 1] offsets of the 64-row blocks
    if (c->d_cell_off.ensure(sizeof(long long) * (size_t)(nb + 1))) return VAG_E_HIP;
    if (c->d_fail.ensure(sizeof(int) * 16)) return VAG_E_HIP;

    // Grid shapes decide the compact layout and the launch geometry of everything downstream.  The last wavefront of
    // vag_grid_kernel scans them on the device and publishes an 80-byte summary in pinned host memory; the host spins on its
    // sequence number (wait_plan: ~6 us after the kernel's end, no copy, no stream synchronisation) and launches the rest.
    // VAG_PLAN_AHEAD=1 instead plans from the previous call's summary with a margin and verifies afterwards
    // (finish_speculation): no host wait in the middle of the pipeline at all.  Measured equal within 3 % in a sampler loop
    // (0.716 vs 0.715 ms per 128-walker call) and slower when calls are queued back to back without reading ln L
    // (0.775 vs 0.693 ms), because its flux launches are sized for the margin -- so waiting is the default.
    static const bool plan_ahead = vag_hook("VAG_PLAN_AHEAD") != nullptr;
    const bool spec = may_plan_ahead(plan_ahead, may_plan, want_details, c->hint_valid, c->hint_nb, nb);
    const StageCaps cap = spec ? plan_ahead_caps(c->hint, c->spec_margin_k) : StageCaps{};
    if (spec) c->spec_cap_k = cap.k;
    if (c->d_plan.ensure(sizeof(VagDevPlan) + 64)) return VAG_E_HIP;
    if (!c->h_plan.p) {  // pinned, host-mapped, COHERENT (fine-grained: a store from a running kernel reaches the host after a
                         // system-scope fence, not only at the end of the queue): the grid kernel's last wavefront writes the
                         // batch summary straight into it
        HIPCHK(hipHostMalloc(&c->h_plan.p, 256, hipHostMallocMapped | hipHostMallocCoherent));
        c->h_plan.cap = 256;
        std::memset(c->h_plan.p, 0, sizeof(VagDevPlan));
        void* dp = nullptr;
        HIPCHK(hipHostGetDevicePointer(&dp, c->h_plan.p, 0));
        c->d_hplan = static_cast<VagDevPlan*>(dp);
    }
    if (!c->plan_counter_ready) {  // the ticket counter behind the plan: zeroed once, the kernel leaves it at zero
        HIPCHK(hipMemsetAsync(reinterpret_cast<char*>(c->d_plan.p) + sizeof(VagDevPlan), 0, 64, st));
        c->plan_counter_ready = true;
    }
    c->ic_need_reset = true;
    c->prof_spans.clear();
    c->prof_used = 0;
    HIPCHK(hipEventRecord(c->ev[0], st));
    std::unique_ptr<StageScope> ps_grid(new StageScope(c, PS_DYNAMICS));  // closed right after the launch below
    auto launch_grid = [&](int large) {
        c->layout_large = large;  // the layout THIS batch is laid out with (c->grid_large may change below for the next one)
        auto kern = large == 2 ? vag_grid_kernel<2> : (large == 1 ? vag_grid_kernel<1> : vag_grid_kernel<0>);
        hipLaunchKernelGGL(kern, dim3(nb), dim3(WAVE), 0, st, d_params, nb, c->d_tminmax.as<double>(),
                           c->d_meta.as<VagGridMeta>(), c->d_phi.as<double>(), c->d_theta.as<double>(), c->d_rep_of.as<int>(),
                           c->d_rep_start.as<int>(), c->d_tdec.as<double>(), c->d_geo_th.as<double>(), c->d_geo_ph.as<double>(),
                           c->d_fail.as<int>(), reinterpret_cast<int*>(reinterpret_cast<char*>(c->d_plan.p) + sizeof(VagDevPlan)),
                           c->d_row_off.as<int>(), c->d_cell_off.as<long long>(), c->d_plan.as<VagDevPlan>(), c->d_hplan, ++c->plan_seq,
                           cap.rows, cap.cells, cap.k, cap.pairs, spec ? plan_flags(c->hint) : -1,
                           spec ? c->hint.dyn_class : 0, c->d_cost_f.as<float>(), c->d_rowgeo.as<double>(),
                           large == 2 ? c->d_gridscratch.as<GridSharedHuge>() : nullptr);
    };
    launch_grid(c->grid_large);
    ps_grid.reset();
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[1], st));
    long long cells, pairs, eat;
    int rows, max_k, max_pairs, n_ok, n_invalid = 0, n_capacity = 0, dyn_class, flags;
    c->spec_pending = false;
    if (!spec) {
        VagDevPlan* hp = c->h_plan.as<VagDevPlan>();
        if (int rcw = wait_plan(c)) return rcw;
        // some model's angular grid outgrew the layout of the grid kernel: lay the batch out again with the next one (the same grids
        // for every model that fitted), and keep using it while the caller keeps sending such models
        while (hp->n_capacity > 0 && c->grid_large < 2) {
            ++c->grid_large;
            HIPCHK(hipStreamSynchronize(st));  // (the arrays are about to be re-allocated at the larger stride; nothing may still write them)
            if (ensure_angular(c->grid_large)) return VAG_E_HIP;
            if (vag_hook("VAG_DEBUG_LAUNCH"))
                std::fprintf(stderr, "[vag] grid: %d of %d models over the capacity of layout %d, laying the batch out again\n", hp->n_capacity, nb,
                             c->grid_large - 1);
            launch_grid(c->grid_large);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(c->ev[1], st));
            if (int rcw = wait_plan(c)) return rcw;
        }
        if (hp->n_capacity == 0 && c->grid_large && c->layout_large == c->grid_large && ++c->grid_large_idle >= 8) {
            c->grid_large = 0;  // eight batches in a row fitted: back to the small layout (several models per CU)
            c->grid_large_idle = 0;
        }
        if (hp->n_capacity > 0) c->grid_large_idle = 0;
        c->mixed_flags_seen = hp->flags_mixed != 0;
        if (hp->flags_mixed)
            return set_err(VAG_E_UNSUPPORTED, "models with different Radiation / shock flags in one device-resident batch: split it by flags "
                                              "(the flux entry points do that themselves)");
        rows = hp->rows, cells = hp->cells, pairs = hp->pairs, eat = hp->eat, max_k = hp->max_k, max_pairs = hp->max_pairs;
        n_ok = hp->n_ok, n_invalid = hp->n_invalid, n_capacity = hp->n_capacity, dyn_class = hp->dyn_class;
        flags = plan_flags(*hp);
        c->hint = *hp;
        c->hint_nb = nb;
        c->hint_valid = hp->n_ok > 0;
    } else {  // launch geometry and strides from the capacities, kernel choice from the previous call's flags
        rows = cap.rows, cells = cap.cells, max_k = cap.k, max_pairs = cap.pairs;
        pairs = c->hint.pairs, eat = c->hint.eat, n_ok = c->hint.n_ok, dyn_class = c->hint.dyn_class;
        flags = plan_flags(c->hint);
        c->spec_pending = true;
    }
    c->batch_flags = flags;
    // (A spreading jet under axisymmetric=False has one time lattice and one ODE solve per (phi, theta) node, grid-refinement.h:619-625:
    // the ODE rows are (phi, theta) pairs, VagGridMeta::rep_phi_stride.)
    c->nb = nb;
    c->n_rows = rows;
    c->n_cells = cells;
    c->max_k = max_k;
    c->max_pairs = max_pairs;
    c->total_pairs = pairs;
    c->eat_cells = eat;
    c->n_ok = n_ok;
    c->plan = vag_plan{};
    c->fit_stats_pending = false;
    c->ic_slow_unread = false;
    c->plan.n_models_ok = n_ok;
    c->plan.n_rows = rows;
    c->plan.n_cells = cells;
    c->plan.total_pairs = pairs;
    c->plan.eat_cells = eat;
    c->plan.n_models_invalid = n_invalid;
    c->plan.n_models_capacity = n_capacity;
    c->meta_on_host = false;
    if (rows == 0) {
        HIPCHK(hipEventRecord(c->ev[2], st));
        HIPCHK(hipEventRecord(c->ev[3], st));
        return VAG_OK;
    }
    const DynHooks dyn_hk = dyn_hooks();
    const DynPlan dyn = dyn_plan(c->batch_flags, dyn_class, rows, c->n_cus, dyn_hk);  // which solver, how many rows per wavefront
    const bool rvs = dyn.family == DYN_PAIR, spreading = dyn.spreading;
    const int rpw = dyn.rows_per_wave;
    if (c->d_shock.ensure(sizeof(double) * (size_t)cells * VAG_NSHOCK)) return VAG_E_HIP;
    if (c->d_row_status.ensure(sizeof(int) * (size_t)rows)) return VAG_E_HIP;
    Layout lay{c->d_row_off.as<int>(), c->d_cell_off.as<long long>()};
    bool raw_shock = false;
    std::unique_ptr<StageScope> ps_dyn(new StageScope(c, PS_DYNAMICS));
    if (rvs) {  // generate_shock_pair (reverse-shock.tpp:592-614): both shocks from one ODE state per row
        if (c->d_shock_r.ensure(sizeof(double) * (size_t)cells * VAG_NSHOCK)) return VAG_E_HIP;
        if (c->d_inj.ensure(sizeof(int) * (size_t)rows)) return VAG_E_HIP;
        if (c->d_params_rvs.ensure(sizeof(vag_model_params) * (size_t)nb)) return VAG_E_HIP;
        hipLaunchKernelGGL(vag_rvs_params_kernel, dim3((nb + 127) / 128), dim3(128), 0, st, d_params, nb,
                           c->d_params_rvs.as<vag_model_params>());
        hipLaunchKernelGGL(vag_dynamics_pair_kernel, dim3((rows + rpw - 1) / rpw), dim3(64), 0, st, d_params, nb,
                           c->d_meta.as<VagGridMeta>(), c->d_theta.as<double>(), c->d_rep_start.as<int>(),
                           c->d_tdec.as<double>(), lay, rows, c->d_shock.as<double>(), c->d_shock_r.as<double>(), cells,
                           c->d_inj.as<int>(), c->d_row_status.as<int>(), c->d_fail.as<int>(), c->d_phi.as<double>(),
                           c->d_tminmax.as<double>(), rpw);
    } else if (dyn.family != DYN_GENERAL) {  // the common case: flat attempt loop, raw saves
        raw_shock = true;
        if (dyn.family == DYN_REFILL) {  // the rows are queued longest first (vag_dyn_fast.h: a row's step count is predictable from its start record), by a counting sort of three small kernels
            const DynRecLayout l = dynrec_layout(rows, {DYN_ROWREC, DYN_BUCKETS, DYN_CHUNK});
            const size_t n_chunks = l.n_chunks;
            if (c->d_dynrec.ensure(l.bytes)) return VAG_E_HIP;
            char* dyn_base = static_cast<char*>(c->d_dynrec.p);
            int* d_dynorder = reinterpret_cast<int*>(dyn_base + l.order);
            unsigned* d_queue = reinterpret_cast<unsigned*>(dyn_base + l.queue);
            unsigned* d_hist = reinterpret_cast<unsigned*>(dyn_base + l.hist);
            signed char* d_cls = reinterpret_cast<signed char*>(dyn_base + l.cls);
            hipLaunchKernelGGL(vag_dyn_prep_kernel, dim3((unsigned)n_chunks), dim3(DYN_CHUNK), 0, st, d_params, nb, c->d_meta.as<VagGridMeta>(),
                               c->d_theta.as<double>(), c->d_rep_start.as<int>(), c->d_tdec.as<double>(), lay, rows, c->d_shock.as<double>(), cells,
                               c->d_row_status.as<int>(), c->d_dynrec.as<double>(), d_cls, d_hist);
            hipLaunchKernelGGL(vag_dyn_scan_kernel, dim3(1), dim3(1024), 0, st, d_hist, (int)n_chunks, d_queue);
            hipLaunchKernelGGL(vag_dyn_file_kernel, dim3((unsigned)n_chunks), dim3(DYN_CHUNK), 0, st, d_cls, d_hist, rows, d_dynorder);
            auto kern = c->count_work ? vag_dynamics_refill_kernel<true> : vag_dynamics_refill_kernel<false>;
            if (c->dyn_refill_wg_per_cu <= 0) {  // what the registers allow (two wavefronts per SIMD at <= 256 VGPRs)
                int per_cu = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, vag_dynamics_refill_kernel<false>, 64, 0) != hipSuccess || per_cu <= 0) per_cu = 8;
                c->dyn_refill_wg_per_cu = per_cu;
            }
            const unsigned wgs = refill_workgroups(rows, c->dyn_refill_wg_per_cu, c->n_cus, dyn_hk.refill_wgs);
            hipLaunchKernelGGL(kern, dim3(wgs), dim3(64), 0, st, c->d_dynrec.as<double>(), rows, c->d_shock.as<double>(), cells,
                               c->d_row_status.as<int>(), c->d_sptab.as<double>(), dyn.refill_min, c->d_fail.as<int>(), d_queue, d_dynorder);
        } else {
        hipLaunchKernelGGL(c->count_work ? vag_dynamics_fast_kernel<true> : vag_dynamics_fast_kernel<false>, dim3((rows + rpw - 1) / rpw),
                           dim3(128), 0, st, d_params, nb, c->d_meta.as<VagGridMeta>(), c->d_theta.as<double>(), c->d_rep_start.as<int>(),
                           c->d_tdec.as<double>(), lay, rows, c->d_shock.as<double>(), cells, c->d_row_status.as<int>(),
                           c->d_sptab.as<double>(), rpw, c->d_fail.as<int>());
        }
    } else {
        auto kern = spreading ? (dyn.inject ? vag_dynamics_kernel<true, true> : vag_dynamics_kernel<true, false>)
                              : (dyn.inject ? vag_dynamics_kernel<false, true> : vag_dynamics_kernel<false, false>);
        hipLaunchKernelGGL(kern, dim3((rows + rpw - 1) / rpw), dim3(64), 0, st, d_params, nb, c->d_meta.as<VagGridMeta>(),
                           c->d_theta.as<double>(), c->d_rep_start.as<int>(), c->d_tdec.as<double>(), lay, rows,
                           c->d_shock.as<double>(), cells, c->d_row_status.as<int>(), c->d_sptab.as<double>(), rpw,
                           c->d_fail.as<int>(), c->d_phi.as<double>(), c->d_tminmax.as<double>());
    }
    HIPCHK(hipGetLastError());
    if (spreading) {  // per-cell viewing geometry from the evolved theta (both shocks ride the same contact discontinuity)
        if (c->d_cellgeo.ensure(sizeof(double) * (size_t)cells * 3)) return VAG_E_HIP;
        hipLaunchKernelGGL(vag_spread_geo_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, nb,
                           c->d_meta.as<VagGridMeta>(), lay, c->d_shock.as<double>(), cells, c->d_cellgeo.as<double>());
        HIPCHK(hipGetLastError());
    }
    ps_dyn.reset();
    HIPCHK(hipEventRecord(c->ev[2], st));
    c->cur_emitter = 0;
    c->cur_params = d_params;
    c->cur_ssc = (c->batch_flags & VAG_FLAG_SSC) != 0;
    int rc = run_radiation(c, d_params, nb, nullptr, c->cur_ssc, want_details, raw_shock);
    if (rc) return rc;
    if (rvs) {
        select_emitter(c, 1, d_params);
        rc = run_radiation(c, c->cur_params, nb, c->d_inj.as<int>(), c->cur_ssc, want_details);
        select_emitter(c, 0, d_params);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(c->ev[3], st));
    return VAG_OK;
}

// ---- the flux launch layer.  What is launched is decided in vag_flux_plan.h (host arithmetic, tested on the CPU); here are the
//      inputs of those decisions, one selector per kernel family that maps a variant to its kernel, and the launches ----

static FluxBatch flux_batch(const vag_ctx* c, int nb) {  // (FluxBatch's members in their order)
    return {nb,        c->n_rows,     c->max_k,   c->max_pairs, c->total_pairs,
            c->n_cus,  c->count_work, c->ppb_pin, (c->batch_flags & VAG_FLAG_SPREADING) != 0};
}

static FluxHooks flux_hooks() {  // (FluxHooks' members in their order)
    const auto get = hook_int;
    return {get("VAG_PAIRS_PER_BLOCK"), get("VAG_FLUX_K_CAP"), get("VAG_FLUX_WIDE"), get("VAG_GRID_ROWWISE"),
            get("VAG_GRID_ROW_PER_WORKGROUP"), get("VAG_FLUX_PERSISTENT"), get("VAG_FLUX_SPLIT"), get("VAG_NO_FUSED"),
            get("VAG_FORCE_FUSED"), get("VAG_SERIES_ROW_PER_WAVE"), get("VAG_FIT_WAVES_PER_BLOCK"), get("VAG_SERIES_PPB"),
            get("VAG_SERIES_WAVES")};
}

static int flux_ks(const vag_ctx* c) { return flux_ks(flux_batch(c, 0), flux_hooks()); }

// The batch's device pointers that every flux and sky argument struct carries (FluxArgs, SeriesArgs, SkyArgs, SkyCenArgs: a new
// per-batch buffer is bound here, once).  d_params: of the selected emitter.  The row / cell offsets differ per struct and stay
// with the caller (bind_layout), as do the request's own members.  The SSC tables' three pointers are valid only behind the table
// build, which may reallocate them: a caller that builds tables after this binds those three again.
template <class A>
static void bind_batch(A& a, const vag_ctx* c, const vag_model_params* d_params) {
    a.params = d_params;
    a.meta = c->d_meta.as<VagGridMeta>();
    a.geo_th = c->d_geo_th.as<double>();
    a.geo_ph = c->d_geo_ph.as<double>();
    a.g_rep_of = c->d_rep_of.as<int>();
    a.cellpar = c->d_cellpar.as<double>();
    a.cellq = c->d_cellq.as<double>();
    a.cellgeo = c->d_cellgeo.as<double>();
    a.sp_table = c->d_sptab.as<double>();
    a.ichdr = c->d_ichdr.as<double>();
    a.icpool = c->d_icpool.as<double>();
    a.ic_status = c->d_icstatus.as<int>();
}
template <class A>
static void bind_layout(A& a, const vag_ctx* c) { a.cell_off = c->d_cell_off.as<long long>(); }
static void bind_layout(SeriesArgs& a, const vag_ctx* c) { a.lay = Layout{c->d_row_off.as<int>(), c->d_cell_off.as<long long>()}; }

// Resident workgroups per CU of `fn` with `threads` lanes and `lds` bytes: the occupancy query, remembered per shape; -1 where the
// query fails.  raise_lds: the kernel's dynamic-LDS limit is lifted to a CU's before the first query.
static int wg_per_cu(vag_ctx* c, const void* fn, int threads, size_t lds, bool raise_lds = false) {
    for (const auto& e : c->occ)
        if (e.fn == fn && e.threads == threads && e.lds == lds) return e.wg;
    int wg = -1;
    if (raise_lds) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)CU_LDS_BYTES);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&wg, fn, threads, lds) != hipSuccess) wg = -1;
    if (c->occ.size() > 256) c->occ.clear();
    c->occ.push_back({fn, threads, lds, wg});
    return wg;
}

// the work-item counter of a persistent launch (SeriesArgs::work), in the zeroed words behind the device plan: the kernel behind every
// such launch puts it back to zero, and kernels of one context run on one stream
static int* work_counters(vag_ctx* c) { return reinterpret_cast<int*>(reinterpret_cast<char*>(c->d_plan.p) + sizeof(VagDevPlan)) + 4; }

// dynamic LDS of vag_flux_grid_kernel (layout at the top of the kernel)
static size_t flux_grid_lds_bytes(int mode, int ks, int nt, int nnu) {
    const size_t slots = (size_t)nt * nnu;
    size_t d = (size_t)(VAG_NPAR + 4) * ks + (size_t)ks * nnu + 2 * (size_t)nt + nnu + SP_LDS_DOUBLES + slots;
    if (mode == FLUX_FUSED) d += 6 * (size_t)ks + (size_t)ks * nnu + slots;
    return sizeof(double) * d + sizeof(int) * nt + 16;  // + s_win: [2][2] observation-window counts (WinCount)
}

// Stage 4-5 for a (t, nu) grid request: d_lg2t/d_lg2nu are log2 of code-unit times / frequencies.
int run_flux_series(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, const double* d_lg2nu, int n,
                    double* d_out, int mode = FLUX_SYN, int n_bands = 0, int grid_nt = 0);

// fixed-order sum of a flux pass's workgroup partials + normalisation: plain grids through the grouped kernel, band-weighted
// requests through the serial one
static void launch_reduce(hipStream_t st, const vag_model_params* d_params, const VagGridMeta* meta, const double* partial, int max_blocks,
                          int ppb, int nt, int nnu, const double* d_bandw, double* d_out, int nb,
                          int* work_counter = nullptr /* of a persistent flux launch before this one: the reduction puts it back to zero */) {
    if (d_bandw) {
        hipLaunchKernelGGL(vag_reduce_kernel, dim3((nt + 255) / 256, nb), dim3(256), 0, st, d_params, meta, partial, max_blocks, ppb, nt, nnu,
                           d_bandw, d_out, work_counter);
    } else {
        const int slots = nt * nnu;
        hipLaunchKernelGGL(vag_reduce_grid_kernel, dim3((slots + REDUCE_SLOTS - 1) / REDUCE_SLOTS, nb), dim3(REDUCE_GROUPS * REDUCE_SLOTS), 0, st,
                           d_params, meta, partial, max_blocks, ppb, slots, d_out, work_counter);
    }
}

// The workgroup kernel of a grid request: the 21 variants grid_variant can give, each as the kernel of one item per workgroup and
// as the persistent one (42 kernels; what is not listed is not instantiated).
using FluxKernel = void (*)(FluxArgs);
struct GridKernels {
    FluxKernel one = nullptr, persistent = nullptr;
};
template <bool COUNT, int MODE, bool SPREAD = false, int THREADS = FLUX_THREADS, bool PIECES = false>
static GridKernels grid_pair() {
    return {vag_flux_grid_kernel<COUNT, MODE, SPREAD, THREADS, PIECES>, vag_flux_grid_kernel<COUNT, MODE, SPREAD, THREADS, PIECES, true>};
}
constexpr int grid_key(int mode, bool spread, int lanes, bool pieces, bool count = false) {
    return mode | (spread ? 4 : 0) | (lanes == 256 ? 8 : 0) | (pieces ? 16 : 0) | (count ? 32 : 0);
}
static GridKernels grid_kernels(const GridVariant& v) {
    constexpr int W = FLUX_THREADS;
    switch (grid_key(v.mode, v.spread, v.lanes, v.pieces, v.count)) {
        case grid_key(FLUX_SYN, false, W, false): return grid_pair<false, FLUX_SYN>();
        case grid_key(FLUX_SYN_IC, false, W, false): return grid_pair<false, FLUX_SYN_IC>();
        case grid_key(FLUX_SSC, false, W, false): return grid_pair<false, FLUX_SSC>();
        case grid_key(FLUX_FUSED, false, W, false): return grid_pair<false, FLUX_FUSED>();
        case grid_key(FLUX_SYN, false, W, false, true): return grid_pair<true, FLUX_SYN>();
        case grid_key(FLUX_SYN, true, W, false): return grid_pair<false, FLUX_SYN, true>();
        case grid_key(FLUX_SYN_IC, true, W, false): return grid_pair<false, FLUX_SYN_IC, true>();
        case grid_key(FLUX_SSC, true, W, false): return grid_pair<false, FLUX_SSC, true>();
        case grid_key(FLUX_FUSED, true, W, false): return grid_pair<false, FLUX_FUSED, true>();
        case grid_key(FLUX_SYN, false, 256, false): return grid_pair<false, FLUX_SYN, false, 256>();
        case grid_key(FLUX_SYN_IC, false, 256, false): return grid_pair<false, FLUX_SYN_IC, false, 256>();
        case grid_key(FLUX_SSC, false, 256, false): return grid_pair<false, FLUX_SSC, false, 256>();
        case grid_key(FLUX_FUSED, false, 256, false): return grid_pair<false, FLUX_FUSED, false, 256>();
        case grid_key(FLUX_SYN, false, W, true): return grid_pair<false, FLUX_SYN, false, W, true>();
        case grid_key(FLUX_SYN_IC, false, W, true): return grid_pair<false, FLUX_SYN_IC, false, W, true>();
        case grid_key(FLUX_SSC, false, W, true): return grid_pair<false, FLUX_SSC, false, W, true>();
        case grid_key(FLUX_FUSED, false, W, true): return grid_pair<false, FLUX_FUSED, false, W, true>();
        case grid_key(FLUX_SYN, true, W, true): return grid_pair<false, FLUX_SYN, true, W, true>();
        case grid_key(FLUX_SYN_IC, true, W, true): return grid_pair<false, FLUX_SYN_IC, true, W, true>();
        case grid_key(FLUX_SSC, true, W, true): return grid_pair<false, FLUX_SSC, true, W, true>();
        case grid_key(FLUX_FUSED, true, W, true): return grid_pair<false, FLUX_FUSED, true, W, true>();
    }
    return {};
}

// vag_flux_grid_rows_kernel: one instantiation per photon source (3)
using SeriesKernel = void (*)(SeriesArgs);
static SeriesKernel grid_rows_kernel(int mode) {
    switch (mode) {
        case FLUX_SYN_IC: return vag_flux_grid_rows_kernel<FLUX_SYN_IC>;
        case FLUX_SSC: return vag_flux_grid_rows_kernel<FLUX_SSC>;
        default: return vag_flux_grid_rows_kernel<FLUX_SYN>;
    }
}

// One launch over the work items of `a` (a.n_items = models x blocks): a workgroup per item with `one`, or -- where persist_plan
// says so -- the persistent kernel `pers` with as many workgroups as stay resident, its items dealt by descending model cost
// (vag_flux_order_kernel).  one == nullptr (the split form, which has no one-item kernel): nothing is launched where the launch
// does not go persistent.  Returns whether it took the persistent form (its counter then has to go back to zero behind it).
static bool launch_flux_items(vag_ctx* c, FluxArgs a, int nb, FluxKernel one, FluxKernel pers, int threads, size_t lds, int persist) {
    const bool debug = vag_hook("VAG_DEBUG_LAUNCH") != nullptr;
    // (a failed query counts as one resident workgroup; the present kernel's LDS limit is lifted with its first query, as it always was)
    const int wg = persist ? std::max(1, wg_per_cu(c, reinterpret_cast<const void*>(pers), threads, lds, one != nullptr)) : -1;
    const PersistPlan p = persist_plan(persist, a.n_items, wg, c->n_cus, a.pairs_per_block);
    if (!p.persistent) {
        if (!one) return false;
        if (debug) std::fprintf(stderr, "[vag] grid flux form: one item per workgroup, %d x %d\n", a.max_blocks, nb);
        a.work = nullptr;
        hipLaunchKernelGGL(one, dim3(a.max_blocks, nb), dim3(threads), lds, c->stream, a);
        return false;
    }
    if (debug) {
        std::fprintf(stderr, "[vag] grid flux form: persistent, %lld workgroups for %d items\n", p.n_wg, a.n_items);
        if (!one)
            std::fprintf(stderr, "[vag] grid flux split: %d + %d wavefronts (boundary spectra + interpolation), lds=%zu B wg/CU=%d\n", FLUX_SPLIT_A,
                         FLUX_SPLIT_B, lds, wg);
    }
    hipLaunchKernelGGL(vag_flux_order_kernel, dim3((nb + 3) / 4), dim3(256), 0, c->stream, a.meta, nb, const_cast<int*>(a.order));
    hipLaunchKernelGGL(pers, dim3((unsigned)p.n_wg), dim3(threads), lds, c->stream, a);
    return true;
}

int run_flux_grid(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, int nt,
                  const double* d_lg2nu, int nnu, const double* d_bandw, double* d_out, int mode = FLUX_SYN,
                  double* d_out2 = nullptr /* FLUX_FUSED: the SSC component */) {
    hipStream_t st = c->stream;
    StageScope ps(c, mode == FLUX_SSC ? PS_SSC_FLUX : PS_SYNC_FLUX);
    const int slots = nt * nnu;
    const FluxBatch batch = flux_batch(c, nb);
    const FluxHooks hooks = flux_hooks();
    const bool debug = vag_hook("VAG_DEBUG_LAUNCH") != nullptr;
    // Rows of a few hundred (nu, t) slots keep a 256-lane workgroup 22-78 % busy between its two barriers (C3, C5, C1: four or
    // three frequencies).  The wavefront-per-row kernel can serve them (VAG_GRID_ROWWISE=1: same algorithm -- boundary spectra
    // per (nu, lattice node of the window), log-log interpolation --, no workgroup barrier, accumulators in registers), but
    // MEASURED SLOWER on every such shape (C5 2.2 k vs 4.5 k light curves/s, C3 1.27 k vs 1.79 k, C1a 1.28 M vs 2.58 M: eight
    // points per lane cost the occupancy, and every lane walks its own bracket searches), so the workgroup kernel stays.
    if (grid_rowwise(batch, hooks, mode, nt, nnu, d_bandw != nullptr))
        return run_flux_series(c, d_params, nb, d_lg2t, d_lg2nu, slots, d_out, mode, nnu, nt);
    if (slots > FLUX_MAX_SLOTS)
        return set_err(VAG_E_CAPACITY, "nt*nnu = %d exceeds %d per launch", slots, FLUX_MAX_SLOTS);
    if (const GridRowsPlan p = grid_rows_plan(batch, hooks, mode, nt, nnu); p.take) {  // a (theta, phi) row per lane (vag_grid_rows.h)
        if (c->d_partial.ensure(sizeof(double) * (size_t)nb * p.max_blocks * slots)) return VAG_E_HIP;
        SeriesArgs a{};
        bind_batch(a, c, d_params);
        bind_layout(a, c);
        a.cellgeo = nullptr;  // (never a spreading batch)
        a.lg2_t_obs = d_lg2t;
        a.lg2_nu_obs = d_lg2nu;
        a.n = slots;
        a.grid_nt = nt;
        a.n_bands = nnu;
        a.max_chunks = p.max_blocks;
        a.partial = c->d_partial.as<double>();
        c->plan.spec_evals += c->eat_cells * nnu;
        c->plan.interps += c->total_pairs * (long long)nt * nnu;
        c->plan.flux_blocks = p.max_blocks * nb;
        c->plan.pairs_per_block = FITROWS_ROWS;
        a.nb = nb;
        a.work = work_counters(c);
        const size_t lds = grid_rows_lds_bytes(slots);
        if (debug)
            std::fprintf(stderr, "[vag] grid rows launch: mode %d nt=%d nnu=%d blocks=%lld persistent=%d lds=%zu B\n", mode, nt, nnu, p.blocks,
                         (int)p.persistent, lds);
        hipLaunchKernelGGL(grid_rows_kernel(mode), p.persistent ? dim3(p.wg_persistent) : dim3(p.wg_all, nb),
                           dim3(SERIES_THREADS * GRIDROWS_WAVES), lds, st, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[4], st));
        launch_reduce(st, d_params, c->d_meta.as<VagGridMeta>(), c->d_partial.as<double>(), p.max_blocks, FITROWS_ROWS, nt, nnu, d_bandw, d_out,
                      nb, p.persistent ? work_counters(c) : nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[5], st));
        return VAG_OK;
    }
    const int ppb = choose_pairs_per_block(batch, hooks);
    const int max_blocks = std::max(1, (c->max_pairs + ppb - 1) / ppb);
    if (c->d_partial.ensure(sizeof(double) * (size_t)nb * max_blocks * slots)) return VAG_E_HIP;
    const int ks = flux_ks(batch, hooks);
    const size_t lds = flux_grid_lds_bytes(mode, ks, nt, nnu);
    if (lds > CU_LDS_BYTES) return set_err(VAG_E_CAPACITY, "LDS request %zu B exceeds 160 KiB (n_t=%d, nnu=%d)", lds, ks, nnu);
    if (mode == FLUX_FUSED && c->d_partial2.ensure(sizeof(double) * (size_t)nb * max_blocks * slots)) return VAG_E_HIP;
    const GridVariant v = grid_variant(batch, hooks, mode, nt, nnu, ks);
    FluxArgs a{};  // (work_count, rowgeo, work and order stay null where nothing below sets them)
    bind_batch(a, c, d_params);
    bind_layout(a, c);
    a.lg2_t_obs = d_lg2t;
    a.lg2_nu_obs = d_lg2nu;
    a.nt = nt;
    a.nnu = nnu;
    a.pairs_per_block = ppb;
    a.max_blocks = max_blocks;
    a.k_stride = ks;
    a.partial = c->d_partial.as<double>();
    a.partial2 = c->d_partial2.as<double>();
    a.n_items = nb * max_blocks;
    if (!batch.spreading) {  // the models' row-geometry records, written by the grid kernel with the layout it ran with
        a.rowgeo = c->d_rowgeo.as<double>();
        a.rowgeo_stride = rowgeo_stride(c->layout_large);
    }
    if (v.count) {
        if (c->d_workcount.ensure(2 * sizeof(unsigned long long))) return VAG_E_HIP;
        HIPCHK(hipMemsetAsync(c->d_workcount.p, 0, 2 * sizeof(unsigned long long), st));
        a.work_count = c->d_workcount.as<unsigned long long>();
    }
    // upper bounds (every lattice node inside the observation window); vag_ctx_count_work(1) replaces them by
    // the exact tallies of the kernel
    c->plan.spec_evals += c->eat_cells * nnu;
    c->plan.interps += c->total_pairs * (long long)nt * nnu;
    c->plan.flux_blocks = max_blocks * nb;
    c->plan.pairs_per_block = ppb;
    bool persistent = false;
    if (c->n_rows > 0) {
        const GridKernels k = grid_kernels(v);
        if (!k.one) return set_err(VAG_E_INVALID, "no flux grid kernel for mode %d", mode);
        if (debug)  // (lds / wg/CU are the present kernel's also where the split form then takes the launch: its own are on its "grid flux split" line)
            std::fprintf(stderr, "[vag] grid flux launch: mode %d nt=%d nnu=%d ks=%d rows/wg=%d lanes=%d lds=%zu B wg/CU=%d\n", mode, nt, nnu, ks,
                         ppb, v.lanes, lds, wg_per_cu(c, reinterpret_cast<const void*>(k.one), v.lanes, lds));
        // (Measured and rejected, profiles/rejected/vag_flux_wide.h: ONE 1024-lane workgroup per CU sharing the staged row and tables, a
        // second boundary block in the LDS that frees, one barrier per row and balanced slot ownership -- bitwise the same fluxes,
        // 27.0-27.7 ms against 21.7 per 512 C2 models: sixteen wavefronts in lockstep lose the overlap two independent workgroups have.)
        // Persistent launch (VAG_FLUX_PERSISTENT=0: a workgroup per item, the launch before it; =2: persistent whatever the shape):
        // the resident workgroups take the items from a counter, the models by descending cost, so that the launch drains on its
        // cheapest items.
        const int persist = hook_or(hooks.persistent, 1);
        if (persist) {
            if (c->d_flux_order.ensure(sizeof(int) * (size_t)nb)) return VAG_E_HIP;
            a.work = work_counters(c);
            a.order = c->d_flux_order.as<int>();
        }
        // The split form of the headline launch (vag_flux_grid_split_kernel: fixed wavefront roles, one barrier per row) where the
        // request is one it serves and the launch goes persistent (VAG_FLUX_SPLIT=0: never; =2: wherever the split form is legal);
        // FluxSplitLds is its LDS layout
        if (grid_variant_plain(v)) {
            const size_t lds_split = FluxSplitLds(ks, nt, nnu).bytes;
            if (split_takes(hook_or(hooks.split, 1), persist, a.rowgeo != nullptr, lds_split, nt, nnu, ks))
                persistent = launch_flux_items(c, a, nb, nullptr, vag_flux_grid_split_kernel, FLUX_THREADS, lds_split, persist);
        }
        if (!persistent) persistent = launch_flux_items(c, a, nb, k.one, k.persistent, v.lanes, lds, persist);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev[4], st));
    if (a.work_count) {
        unsigned long long h[2];
        HIPCHK(hipMemcpyAsync(h, c->d_workcount.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        c->plan.spec_evals += (long long)h[0] - c->eat_cells * nnu;
        c->plan.interps += (long long)h[1] - c->total_pairs * (long long)nt * nnu;
    }
    launch_reduce(st, d_params, c->d_meta.as<VagGridMeta>(), c->d_partial.as<double>(), max_blocks, ppb, nt, nnu, d_bandw, d_out, nb,
                  persistent ? a.work : nullptr);
    if (mode == FLUX_FUSED)
        launch_reduce(st, d_params, c->d_meta.as<VagGridMeta>(), c->d_partial2.as<double>(), max_blocks, ppb, nt, nnu, d_bandw, d_out2, nb);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[5], st));
    return VAG_OK;
}

__global__ void vag_add_kernel(double* __restrict__ out, const double* __restrict__ add, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] += add[i];
}

// SSC emission of the whole batch on a (t, nu) grid (single_shock_emission, pybind/pymodel.h:896-919):
// observation band per k -> SSC table per representative cell -> EAT flux integration over the tables.
// rebuild = the pass before this one ended with band breaches (status bit 2): those models' tables are rebuilt unclamped
int build_ssc_tables(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2nu, int nnu, bool rebuild = false) {
    hipStream_t st = c->stream;
    StageScope ps(c, PS_IC_PHOTONS);
    const int band_stride = std::max(c->max_k, 1);  // [nb][2][band_stride]
    if (c->d_band.ensure(sizeof(double) * (size_t)nb * 2 * band_stride)) return VAG_E_HIP;
    if (c->d_ichdr.ensure(sizeof(double) * (size_t)std::max<long long>(c->n_cells, 1) * IC_HDR)) return VAG_E_HIP;
    if (c->d_icplan.ensure(sizeof(double) * (size_t)std::max<long long>(c->n_cells, 1) * IC_PLAN)) return VAG_E_HIP;
    constexpr int IC_SLOW_LIST = 1 << 18;  // cells of one table build that may take the slow path (more: VAG_E_CAPACITY)
    if (c->d_icused.ensure(4 * sizeof(unsigned long long))) return VAG_E_HIP;
    if (c->d_icslow.ensure(sizeof(int) * (size_t)IC_SLOW_LIST)) return VAG_E_HIP;
    if (c->d_icpool.ensure(sizeof(double) * 1024)) return VAG_E_HIP;  // (never null: the empty tables point at its first words)
    if (c->d_icstatus.ensure(sizeof(int) * (size_t)nb)) return VAG_E_HIP;
    if (c->d_icunclamp.ensure(sizeof(int) * (size_t)nb)) return VAG_E_HIP;
    if (rebuild) {
        hipLaunchKernelGGL(vag_ic_unclamp_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, c->d_icstatus.as<int>(),
                           c->d_icunclamp.as<int>(), nb);
    } else {
        if (!c->ic_soft_fail || c->ic_need_reset)  // a likelihood pass ORs the failures of both shocks' tables into one status per walker
            HIPCHK(hipMemsetAsync(c->d_icstatus.p, 0, sizeof(int) * (size_t)nb, st));
        HIPCHK(hipMemsetAsync(c->d_icunclamp.p, 0, sizeof(int) * (size_t)nb, st));
    }
    c->ic_need_reset = false;
    if (c->n_rows > 0) {
        Layout lay{c->d_row_off.as<int>(), c->d_cell_off.as<long long>()};
        double narrow = 1.0;  // test hook: VAG_DEBUG_IC_NARROW=<factor> shrinks the clamp so that the flux pass breaches it
        if (const char* e = vag_hook("VAG_DEBUG_IC_NARROW")) narrow = std::atof(e);
        // tables only for the cells some row's observation window touches (the reference builds a cell's spectrum on its first
        // query); VAG_IC_ALL_CELLS=1 builds every cell's table (developer aid: A/B timing, and the loud-fault test)
        unsigned char* d_need = nullptr;
        double need_shrink = 1.0;  // test hook: VAG_DEBUG_IC_NEED_SHRINK=<factor> cuts the window short, so that a flux pass meets a skipped cell
        if (const char* e = vag_hook("VAG_DEBUG_IC_NEED_SHRINK")) need_shrink = std::atof(e);
        // (A likelihood call keeps every table: there a model's SSC status folds into the walker's score -- ic_soft_fail, -inf -- so a cell
        // wrongly left without a table would be a silent wrong answer instead of VAG_E_INTERNAL; round 4's sweeps found two such holes
        // in the range test, both on grid requests, both loud.)
        if (!vag_hook("VAG_IC_ALL_CELLS") && !c->ic_all_cells && c->d_tminmax.p && !c->ic_soft_fail) {
            if (c->d_icneed.ensure((size_t)std::max<long long>(c->n_cells, 1))) return VAG_E_HIP;
            HIPCHK(hipMemsetAsync(c->d_icneed.p, 0, (size_t)std::max<long long>(c->n_cells, 1), st));
            d_need = c->d_icneed.as<unsigned char>();
        }
        const bool huge = c->layout_large == 2;  // (the rows' viewing-cosine extrema then go through HBM: the scratch of the grid kernel is free by now)
        hipLaunchKernelGGL(huge ? vag_ic_band_kernel<true> : vag_ic_band_kernel<false>, dim3(nb), dim3(64), 0, st, d_params, c->d_meta.as<VagGridMeta>(),
                           c->d_geo_th.as<double>(), c->d_geo_ph.as<double>(), c->d_rep_of.as<int>(),
                           c->d_cell_off.as<long long>(), c->d_cellpar.as<double>(), d_lg2nu, nnu, c->d_band.as<double>(),
                           (c->batch_flags & VAG_FLAG_SPREADING) ? c->d_cellgeo.as<double>() : nullptr,
                           c->d_icunclamp.as<int>(), narrow, band_stride, c->d_tminmax.as<double>(), d_need, need_shrink,
                           huge ? c->d_gridscratch.as<double>() : nullptr);
        HIPCHK(hipGetLastError());
        if (c->count_work) {
            if (c->d_icwork.ensure(2 * sizeof(unsigned long long))) return VAG_E_HIP;
            HIPCHK(hipMemsetAsync(c->d_icwork.p, 0, 2 * sizeof(unsigned long long), st));
        }
        // {doubles of the pool in use: its first two words serve the gathers of the cells without a table; plan records written; doubles
        // and records of the cells on the slow path}
        static const unsigned long long ic_counters_start[4] = {2, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(c->d_icused.p, ic_counters_start, sizeof ic_counters_start, hipMemcpyHostToDevice, st));
        // The pool grows to what the plan handed out (grow-only: in a sampler's loop it stops growing after a few calls).  The host has
        // to see the total before the spectrum kernel may write: one 32-byte copy and a wait per table build (~20 us against the
        // milliseconds of the build; a grid / series SSC pass ends with such a wait anyway, check_ic_status).  A LIKELIHOOD call has no
        // host wait anywhere in its SSC stage (its table status folds into the walker's score on the device), so it does not get one
        // here either: the pool is sized for the worst case -- every cell a table of IC_MAX_OUT nodes, plus a fixed reserve for the
        // cells of the slow path -- once, the launch covers every cell and the kernels read the record counts from HBM.  That worst case
        // is ~1.5 KB per cell where the tables use ~0.5 KB, and the pool is grow-only and per context: beyond 4 GB of worst case (~2.7 M
        // cells, e.g. 1500 walkers of the configs[3] grid) the wait is taken after all and the pool sized by what the plan handed out
        // (32 GB until round 5 -- several contexts, or torch allocations next to one, could run out of HBM to save 20 us).
        constexpr unsigned long long SLOW_RESERVE_NO_WAIT = 8ull << 20;  // doubles (64 MB): ~2000 cells of twice the fast kernel's lattices
        const unsigned long long worst = (unsigned long long)std::max<long long>(c->n_cells, 1) * IC_MAX_OUT + 1024 + SLOW_RESERVE_NO_WAIT;
        const bool no_wait = c->ic_soft_fail && worst * sizeof(double) <= (4ull << 30) && !vag_hook("VAG_IC_POOL_READBACK");
        int fast_nu_max = IC_MAX_NU;  // test hook: VAG_DEBUG_IC_FAST_NU_MAX=<n> sends the cells with longer seed lattices through the slow path (0: all)
        if (const char* e = vag_hook("VAG_DEBUG_IC_FAST_NU_MAX")) fast_nu_max = std::min(std::atoi(e), IC_MAX_NU);
        hipLaunchKernelGGL(vag_ic_plan_kernel, dim3((unsigned)((c->n_cells + 255) / 256)), dim3(256), 0, st, d_params, nb,
                           c->d_meta.as<VagGridMeta>(), lay, c->n_cells, c->d_celldet.as<double>(), c->d_band.as<double>(),
                           c->d_ichdr.as<double>(), c->d_icplan.as<double>(), c->d_icused.as<unsigned long long>(),
                           c->d_icstatus.as<int>(), c->count_work ? c->d_icwork.as<unsigned long long>() : nullptr, band_stride, d_need,
                           fast_nu_max, no_wait ? SLOW_RESERVE_NO_WAIT : ~0ull >> 1, c->d_icslow.as<int>(), IC_SLOW_LIST);
        HIPCHK(hipGetLastError());
        long long n_run = c->n_cells;  // launch size (an upper bound when the host has not seen the count)
        long long n_slow = -1;         // records on the slow path (-1: not seen)
        c->ic_slow_unread = no_wait;
        if (no_wait) {
            if (c->d_icpool.ensure(sizeof(double) * (size_t)worst)) return VAG_E_HIP;
        } else {
            unsigned long long ic_counters[4] = {0, 0, 0, 0};
            HIPCHK(hipMemcpyAsync(ic_counters, c->d_icused.p, sizeof ic_counters, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const unsigned long long pool_used = ic_counters[0];
            n_run = (long long)ic_counters[1];  // cells that get a table: one plan record each
            n_slow = (long long)std::min<unsigned long long>(ic_counters[3], IC_SLOW_LIST);
            c->plan.n_ssc_slow_cells += n_slow;
            if (c->d_icpool.ensure(sizeof(double) * (size_t)(pool_used + pool_used / 16 + 1024))) return VAG_E_HIP;
            c->plan.ic_pool_bytes = std::max<long long>(c->plan.ic_pool_bytes, (long long)(sizeof(double) * pool_used));
        }
        // one wavefront per plan record (= per cell that gets a table); -DVAG_IC_PERSISTENT=1 developer builds: as many wavefronts as the
        // device holds at the kernel's four per SIMD, each taking the records w, w + G, ...
        long long ic_waves = n_run;
#if VAG_IC_PERSISTENT
        ic_waves = (long long)c->n_cus * 4 * VAG_IC_WAVES;
        if (const char* e = vag_hook("VAG_IC_GRID")) ic_waves = std::max(1, std::atoi(e));  // developer aid
#endif
        if (n_run > 0)
        hipLaunchKernelGGL(vag_ic_photon_kernel, dim3((unsigned)std::min<long long>(n_run, ic_waves)), dim3(64), 0, st,
                           IcPhotonArgs{n_run, no_wait ? c->d_icused.as<unsigned long long>() + 1 : nullptr, c->n_cells, c->d_icy.as<double>(),
                                        c->d_cellpar.as<double>(), c->d_cellq.as<double>(), c->d_sptab.as<double>(), c->d_knlut.as<double>(),
                                        c->d_icplan.as<double>(), c->d_icpool.as<double>()});
        HIPCHK(hipGetLastError());
        // the cells beyond the fast kernel's on-chip layout: one wavefront per listed record (a call that did not wait for the count
        // launches a small fixed grid that finds the list empty)
        if (n_slow != 0) {
            const IcPhotonArgs a{n_run, nullptr, c->n_cells, c->d_icy.as<double>(), c->d_cellpar.as<double>(), c->d_cellq.as<double>(),
                                 c->d_sptab.as<double>(), c->d_knlut.as<double>(), c->d_icplan.as<double>(), c->d_icpool.as<double>()};
            hipLaunchKernelGGL(vag_ic_photon_slow_kernel, dim3((unsigned)(n_slow > 0 ? std::min<long long>(n_slow, 8192) : 128)), dim3(64), 0, st,
                               a, c->d_icslow.as<int>(), c->d_icused.as<unsigned long long>() + 3, IC_SLOW_LIST);
            HIPCHK(hipGetLastError());
        }
        if (c->count_work) {
            unsigned long long h[2] = {0, 0};
            HIPCHK(hipMemcpyAsync(h, c->d_icwork.p, sizeof h, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            c->plan.ic_terms += (long long)h[0];
            c->plan.ic_nodes += (long long)h[1];
        }
    }
    return VAG_OK;
}

// > 0: not an error code of the C-ABI -- a flux pass breached a clamped band, the caller rebuilds those tables unclamped and repeats
constexpr int VAG_IC_REBUILD = 1000;
// > 0 as well: a flux pass queried a cell the lazy selection (vag_ic_band_kernel's range test: a superset of the queried cells by
// construction, but round 4's sweeps met two holes in it) had left without a table.  The caller builds EVERY cell's table and repeats the
// pass -- the answer the reference gives -- and the event is counted (vag_plan.n_ssc_all_cell_fallbacks); VAG_E_INTERNAL only if the
// all-cells pass reports a missing table too.
constexpr int VAG_IC_REBUILD_ALL = 1001;
int check_ic_status(vag_ctx* c, int nb) {
    if (c->ic_soft_fail) return VAG_OK;  // vag_fit_back_kernel folds d_icstatus into the walker's validity (-inf), samplers.py:61-70
    hipStream_t st = c->stream;
    std::vector<int> h(nb);
    HIPCHK(hipMemcpyAsync(h.data(), c->d_icstatus.p, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool breach = false, hole = false;
    for (int m = 0; m < nb; ++m) {
        if (h[m] & 1) return set_err(VAG_E_CAPACITY, "model %d: SSC lattices exceed the engine limits", m);
        if (h[m] & 4) {
            if (c->ic_all_cells) return set_err(VAG_E_INTERNAL, "model %d: a flux pass queried an SSC cell that was given no table", m);
            hole = true;
        }
    }
    if (hole) {
        ++c->plan.n_ssc_all_cell_fallbacks;
        if (vag_hook("VAG_DEBUG_IC_NO_FALLBACK"))  // test hook: the loud answer itself
            return set_err(VAG_E_INTERNAL, "a flux pass queried an SSC cell that was given no table (fallback disabled)");
        return VAG_IC_REBUILD_ALL;
    }
    for (int m = 0; m < nb; ++m)
        if (h[m] & 2) {
            breach = true;
            ++c->plan.n_models_ssc_rebuilt;
        }
    return breach ? VAG_IC_REBUILD : VAG_OK;
}

// The attempts of one SSC flux pass: lazily selected tables -> (a hole in the selection: every cell's table) -> (a breach of a
// clamped band: those models' tables unclamped).  `pass(rebuild)` builds the tables and runs the flux pass; returns the C-ABI code.
template <class Pass>
int ssc_attempts(vag_ctx* c, int nb, Pass pass) {
    // (false on entry -- nothing but the loop below sets it, and it is off again behind the pass --, so what the guard puts back is false)
    CallMode<bool> all_cells(c->ic_all_cells, false);
    bool rebuild = false;
    int rc = VAG_OK;
    for (int attempt = 0; attempt < 3; ++attempt) {
        rc = pass(rebuild);
        if (rc) return rc;
        rc = check_ic_status(c, nb);
        if (rc == VAG_IC_REBUILD_ALL) {
            c->ic_all_cells = true;
            rebuild = false;
        } else if (rc == VAG_IC_REBUILD) {
            rebuild = true;
        } else {
            return rc;
        }
    }
    return set_err(VAG_E_NUMERIC, "SSC query outside the band of an unclamped table");
}

// d_lg2nu_all / nnu_all: every frequency of the request (the seed band is clamped over all of them, also when the
// frequency axis is evaluated in chunks)
int run_flux_ssc(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, int nt, const double* d_lg2nu,
                 int nnu, const double* d_bandw, double* d_ssc, const double* d_lg2nu_all, int nnu_all) {
    return ssc_attempts(c, nb, [&](bool rebuild) {
        const int rc = build_ssc_tables(c, d_params, nb, d_lg2nu_all, nnu_all, rebuild);
        return rc ? rc : run_flux_grid(c, d_params, nb, d_lg2t, nt, d_lg2nu, nnu, d_bandw, d_ssc, FLUX_SSC);
    });
}

// Synchrotron (IC-cooled) and SSC components of one emitter in ONE flux pass: the tables are built first, then both
// spectra ride the same EAT logs, bracket search and barriers (the two-pass form pays that row skeleton twice -- 35-45 %
// of a pass on the C5 / C3 shapes).  Falls back to two passes when the doubled buffers would not fit in LDS twice.
static bool fused_fits(vag_ctx* c, int nt, int nnu) {
    const FluxBatch batch = flux_batch(c, 0);
    const FluxHooks hooks = flux_hooks();
    const int ks = flux_ks(batch, hooks);
    return fused_fits(batch, hooks, nt, nnu, flux_grid_lds_bytes(FLUX_FUSED, ks, nt, nnu), flux_grid_lds_bytes(FLUX_SYN_IC, ks, nt, nnu));
}
int run_flux_fused(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, int nt, const double* d_lg2nu,
                   int nnu, const double* d_bandw, double* d_syn, double* d_ssc, const double* d_lg2nu_all, int nnu_all) {
    return ssc_attempts(c, nb, [&](bool rebuild) {
        const int rc = build_ssc_tables(c, d_params, nb, d_lg2nu_all, nnu_all, rebuild);
        return rc ? rc : run_flux_grid(c, d_params, nb, d_lg2t, nt, d_lg2nu, nnu, d_bandw, d_syn, FLUX_FUSED, d_ssc);
    });
}

__global__ void vag_copy_kernel(double* __restrict__ out, const double* __restrict__ src, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) out[i] = src[i];
}

// One request on a (t, nu) grid (or a band when d_bandw != nullptr) for the whole batch; model stages already run.
// Components in FluxDict order {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} (pybind/pybind.cpp:472-483):
// d_comp (optional) -> d_comp[i] != nullptr receives component i, zeros when that component is disabled;
// d_total (optional) receives the sum of the enabled components in PyFlux::calc_total order (pymodel.cpp:350-364).
int grid_request(vag_ctx* c, const vag_model_params* d_params, int nb, int nt, int nnu, const double* d_bandw, double* d_total,
                 double* const* d_comp, int t_off = 0, int nu_off = 0, int nnu_all = 0) {
    // t_off / nu_off: first requested time / frequency of this call, nnu_all: frequencies of the whole request (chunking)
    if (nnu_all == 0) nnu_all = nnu;
    const double* lg2nu_all = c->d_lg2nu.as<double>();
    const double* lg2nu = lg2nu_all + nu_off;
    const size_t n_out = (size_t)nb * (d_bandw ? nt : (size_t)nt * nnu);
    const int n_em = (c->batch_flags & VAG_FLAG_RVS) ? 2 : 1;
    bool first = true;
    int rc = VAG_OK;
    for (int e = 0; e < 2 && rc == VAG_OK; ++e) {
        if (e < n_em) select_emitter(c, e, d_params);
        double* fused_ssc = nullptr;  // set once the fused pass has produced this emitter's SSC component
        for (int pass = 0; pass < 2 && rc == VAG_OK; ++pass) {
            double* dst_comp = d_comp ? d_comp[2 * e + pass] : nullptr;
            const bool enabled = e < n_em && (pass == 0 || c->cur_ssc);
            if (!enabled) {
                if (dst_comp && hipMemsetAsync(dst_comp, 0, sizeof(double) * n_out, c->stream) != hipSuccess) rc = VAG_E_HIP;
                continue;
            }
            double* dst = dst_comp;
            if (pass == 1 && fused_ssc) {
                dst = fused_ssc;
            } else {
                if (!dst) {
                    if (!d_total) continue;  // nobody wants this component
                    if (first) {
                        dst = d_total;
                    } else {
                        if (c->d_ssc.ensure(sizeof(double) * n_out)) {
                            rc = VAG_E_HIP;
                            break;
                        }
                        dst = c->d_ssc.as<double>();
                    }
                }
                const double* lg2t = c->d_lg2t.as<double>() + t_off;
                double* want_ssc = d_comp ? d_comp[2 * e + 1] : nullptr;
                if (pass == 0 && c->cur_ssc && (want_ssc || d_total) && fused_fits(c, nt, nnu)) {
                    if (!want_ssc) {
                        if (c->d_ssc2.ensure(sizeof(double) * n_out)) {
                            rc = VAG_E_HIP;
                            break;
                        }
                        want_ssc = c->d_ssc2.as<double>();
                    }
                    rc = run_flux_fused(c, c->cur_params, nb, lg2t, nt, lg2nu, nnu, d_bandw, dst, want_ssc, lg2nu_all, nnu_all);
                    fused_ssc = want_ssc;
                } else if (pass == 0) {
                    rc = run_flux_grid(c, c->cur_params, nb, lg2t, nt, lg2nu, nnu, d_bandw, dst, c->cur_ssc ? FLUX_SYN_IC : FLUX_SYN);
                } else {
                    rc = run_flux_ssc(c, c->cur_params, nb, lg2t, nt, lg2nu, nnu, d_bandw, dst, lg2nu_all, nnu_all);
                }
                if (rc) break;
            }
            if (d_total) {
                if (first) {
                    if (dst != d_total) hipLaunchKernelGGL(vag_copy_kernel, dim3(256), dim3(256), 0, c->stream, d_total, dst, n_out);
                    first = false;
                } else {
                    hipLaunchKernelGGL(vag_add_kernel, dim3(256), dim3(256), 0, c->stream, d_total, dst, n_out);
                }
                if (hipGetLastError() != hipSuccess) rc = VAG_E_HIP;
            }
        }
    }
    select_emitter(c, 0, d_params);
    return rc;
}

// [nb][rows][n] chunk results -> their place in the [nb][rows_all][nt] output
__global__ void vag_place_kernel(double* __restrict__ dst, const double* __restrict__ src, int rows, int n, int rows_all, int nt,
                                 int row0, int t0, size_t total) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(i % n);
        const size_t r = i / n;
        const int l = (int)(r % rows);
        const size_t m = r / rows;
        dst[(m * rows_all + row0 + l) * nt + t0 + j] = src[i];
    }
}

// grid_request with the frequency axis cut into chunks of <= VAG_MAX_NU and the time axis into chunks whose (nu, t)
// accumulator and boundary values fit the workgroup's LDS (<= 4096 slots, fewer when the lattice is long): outputs are
// assembled into [nb][rows][nt], rows = nnu (1 for a band).
int grid_request_chunked(vag_ctx* c, const vag_model_params* d_params, int nb, int nt, int nnu, const double* d_bandw,
                         double* d_total, double* const* d_comp) {
    const bool any_ssc = (c->batch_flags & (VAG_FLAG_SSC | VAG_FLAG_RVS_SSC)) != 0;
    // a band integrates all of its frequencies in one launch; a grid is cut into near-equal frequency chunks
    const int nu_parts = d_bandw ? 1 : (nnu + VAG_MAX_NU - 1) / VAG_MAX_NU;
    const int nu_chunk = (nnu + nu_parts - 1) / nu_parts;
    int chunk = std::max(1, 4096 / nu_chunk);
    while (chunk > 8 &&
           flux_grid_lds_bytes(any_ssc ? FLUX_SYN_IC : FLUX_SYN, flux_ks(c), std::min(chunk, nt), nu_chunk) > 160 * 1024)
        chunk >>= 1;
    if (nt <= chunk && nu_parts == 1) return grid_request(c, d_params, nb, nt, nnu, d_bandw, d_total, d_comp);
    chunk = std::min(chunk, nt);
    const int rows_all = d_bandw ? 1 : nnu;
    const size_t cap = (size_t)nb * (d_bandw ? 1 : nu_chunk) * chunk;
    DevBuf& tmp = c->d_chunk;  // grow-only context scratch: the stream orders its reuse
    if (tmp.ensure(sizeof(double) * 5 * cap)) return VAG_E_HIP;
    double* t_total = d_total ? tmp.as<double>() : nullptr;
    double* t_comp[4];
    for (int i = 0; i < 4; ++i) t_comp[i] = (d_comp && d_comp[i]) ? tmp.as<double>() + (size_t)(i + 1) * cap : nullptr;
    int rc = VAG_OK;
    for (int l0 = 0; l0 < nnu && rc == VAG_OK; l0 += nu_chunk) {
        const int nl = std::min(nu_chunk, nnu - l0);
        const int rows = d_bandw ? 1 : nl;
        for (int t0 = 0; t0 < nt && rc == VAG_OK; t0 += chunk) {
            const int n = std::min(chunk, nt - t0);
            rc = grid_request(c, d_params, nb, n, d_bandw ? nnu : nl, d_bandw, t_total, d_comp ? t_comp : nullptr, t0, l0, nnu);
            const size_t total = (size_t)nb * rows * n;
            auto put = [&](double* dst, const double* src) {
                if (rc != VAG_OK || !dst) return;
                hipLaunchKernelGGL(vag_place_kernel, dim3(256), dim3(256), 0, c->stream, dst, src, rows, n, rows_all, nt,
                                   d_bandw ? 0 : l0, t0, total);
                if (hipGetLastError() != hipSuccess) rc = VAG_E_HIP;
            };
            put(d_total, t_total);
            for (int i = 0; i < 4; ++i) put(d_comp ? d_comp[i] : nullptr, t_comp[i]);
        }
        if (d_bandw) break;
    }
    return rc;
}

// Sky images / image moments of the whole batch (vag_sky.h); model stages already run, d_lg2t / d_lg2nu prepared.  Every enabled
// (emitter, pass) -- forward synchrotron, forward SSC, reverse synchrotron, reverse SSC, as grid_request runs them -- writes its
// terms into its own slice of one term list, then the deposit and moment kernels read all slices in that fixed order.  The time axis
// is cut into chunks whose term list, images, visibility partials and baselines stay within 256 MB (VAG_SKY_CHUNK_T: a test's
// chunk length).  Host outputs: h_image [nb][nnu][nt][npixel^2], h_outside [nb][nnu][nt], h_moments [nb][nnu][nt][6], vr->vis
// [nb][nnu][nt][nbl][2]; any may be null.
struct SkyVisReq {
    const double* u;  // [nnu][nt][nbl] wavelengths, shared by the batch
    const double* v;
    int nbl;
    double pa;    // [rad]
    double* vis;  // [nb][nnu][nt][nbl][2] (re, im)
};
// Polarization of a sky request: Stokes sums on the sky and / or Stokes maps (then h_image of sky_request is null and fov, npixel are
// the maps').  spec: host [nb][4], b - 1 of the forward and reverse shock, then their Pi_max, defaults resolved.
struct SkyPolReq {
    const double* spec;
    double pa;
    double* stokes;   // [nb][nnu][nt][3] I, Q, U on the sky, or null
    double* image;    // [nb][nnu][nt][3][npixel^2] in the jet frame, or null
    double* outside;  // [nb][nnu][nt][3] in the jet frame, or null
};
struct SkyPass {
    int e, pass;
};
static std::vector<SkyPass> sky_passes(const vag_ctx* c) {
    std::vector<SkyPass> passes;
    const int n_em = (c->batch_flags & VAG_FLAG_RVS) ? 2 : 1;
    for (int e = 0; e < n_em; ++e) {
        passes.push_back({e, 0});
        if (c->batch_flags & (e == 0 ? VAG_FLAG_SSC : VAG_FLAG_RVS_SSC)) passes.push_back({e, 1});
    }
    return passes;
}

// The terms stage of a sky request: the term list of the times t0 .. t0 + n - 1 of the prepared request (d_lg2t / d_lg2nu) for every
// pass, [pass][4][nb * nnu * n][R] in d_skyterms (ensured by the caller).  d_pol: also the polarization list [pass][3][nb * nnu * n][R]
// (the synchrotron passes' slices only; an SSC pass is unpolarized).  Leaves emitter 0 selected.
static int sky_terms_stage(vag_ctx* c, const vag_model_params* d_params, int nb, int t0, int n, int nnu, const std::vector<SkyPass>& passes,
                           int R, int ks, double* d_pol = nullptr) {
    hipStream_t st = c->stream;
    const int n_pass = (int)passes.size();
    const size_t lds = sizeof(double) * ((size_t)SP_LDS_DOUBLES + (size_t)SKY_WAVES * 3 * ks);
    if (lds > 160 * 1024) return set_err(VAG_E_CAPACITY, "sky image: lattices of %d nodes exceed the terms kernel's LDS", ks);
    const bool spreading = (c->batch_flags & VAG_FLAG_SPREADING) != 0;
    const size_t G = (size_t)nb * nnu * n;
    int rc = VAG_OK;
    for (int q = 0; q < n_pass && rc == VAG_OK; ++q) {
        select_emitter(c, passes[q].e, d_params);
        SkyArgs a{};
        bind_batch(a, c, c->cur_params);
        bind_layout(a, c);
        a.lg2_t_obs = c->d_lg2t.as<double>() + t0;
        a.lg2_nu_obs = c->d_lg2nu.as<double>();
        a.nt = n;
        a.nnu = nnu;
        a.R = R;
        a.ks = ks;
        a.terms = c->d_skyterms.as<double>() + (size_t)q * 4 * G * R;
        a.pol = d_pol ? d_pol + (size_t)q * 3 * G * R : nullptr;
        const int mode = passes[q].pass == 1 ? FLUX_SSC : (c->cur_ssc ? FLUX_SYN_IC : FLUX_SYN);
        auto launch = [&](auto kernel) -> int {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipLaunchKernelGGL(kernel, dim3((R + SKY_WAVES - 1) / SKY_WAVES, nb), dim3(64 * SKY_WAVES), lds, st, a);
            HIPCHK(hipGetLastError());
            return VAG_OK;
        };
        auto terms = [&]() -> int {
            StageScope ps(c, mode == FLUX_SSC ? PS_SSC_FLUX : PS_SYNC_FLUX);
            // the table build (re)allocates its buffers: their addresses are taken behind it, at the launch
            a.ichdr = c->d_ichdr.as<double>();
            a.icpool = c->d_icpool.as<double>();
            a.ic_status = c->d_icstatus.as<int>();
            if (mode == FLUX_SSC)
                return spreading ? launch(vag_sky_terms_kernel<FLUX_SSC, true>) : launch(vag_sky_terms_kernel<FLUX_SSC, false>);
            if (d_pol) {
                if (mode == FLUX_SYN_IC)
                    return spreading ? launch(vag_sky_terms_kernel<FLUX_SYN_IC, true, true>)
                                     : launch(vag_sky_terms_kernel<FLUX_SYN_IC, false, true>);
                return spreading ? launch(vag_sky_terms_kernel<FLUX_SYN, true, true>) : launch(vag_sky_terms_kernel<FLUX_SYN, false, true>);
            }
            if (mode == FLUX_SYN_IC)
                return spreading ? launch(vag_sky_terms_kernel<FLUX_SYN_IC, true>) : launch(vag_sky_terms_kernel<FLUX_SYN_IC, false>);
            return spreading ? launch(vag_sky_terms_kernel<FLUX_SYN, true>) : launch(vag_sky_terms_kernel<FLUX_SYN, false>);
        };
        if (mode == FLUX_SSC) {  // the tables clamped to the requested frequencies exactly as a grid call clamps them
            rc = ssc_attempts(c, nb, [&](bool rebuild) {
                const int rb = build_ssc_tables(c, c->cur_params, nb, c->d_lg2nu.as<double>(), nnu, rebuild);
                return rb ? rb : terms();
            });
        } else {
            rc = terms();
        }
    }
    select_emitter(c, 0, d_params);
    return rc;
}

// The polarization leg of a chunk of a sky request, shared by sky_request and the likelihood's polarization groups: what the Stokes
// kernels read of the chunk's term and polarization lists (sky_terms_stage), with the spec [nb][4] on the device.  The caller sets
// the turn by 2 pa, the outputs and, for sums outside an image, fov and npixel.
static SkyPolArgs sky_pol_args(vag_ctx* c, const std::vector<SkyPass>& passes, int nnu, int n, int R, int n_az, int nt_all, int t0,
                               const double* d_pol, const double* d_spec) {
    SkyPolArgs pa{};
    pa.meta = c->d_meta.as<VagGridMeta>();
    pa.phi = c->d_phi.as<double>();
    pa.terms = c->d_skyterms.as<double>();
    pa.pol = d_pol;
    pa.spec = d_spec;
    pa.n_pass = (int)passes.size();
    for (int q = 0; q < pa.n_pass; ++q) pa.pass_em[q] = passes[q].pass == 0 ? passes[q].e : -1;
    pa.nnu = nnu;
    pa.nt = n;
    pa.R = R;
    pa.n_az = n_az;
    pa.nt_all = nt_all;
    pa.t0 = t0;
    pa.fov = 0.0;
    pa.npixel = 1;
    pa.partial = c->d_skypol.as<double>();
    return pa;
}
// vag_sky_stokes_kernel and vag_sky_stokes_combine over the G images of the chunk (d_skypol ensured by the caller)
static int sky_stokes_stage(vag_ctx* c, const SkyPolArgs& pa, size_t G, int n_pblk) {
    hipLaunchKernelGGL(vag_sky_stokes_kernel, dim3((unsigned)G, (unsigned)n_pblk), dim3(64), 0, c->stream, pa);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(vag_sky_stokes_combine, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, pa, (int)G);
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

int sky_request(vag_ctx* c, const vag_model_params* d_params, int nb, int nt, int nnu, int n_az, double fov, int npixel,
                double* h_image, double* h_outside, double* h_moments, const SkyVisReq* vr = nullptr, const SkyPolReq* pr = nullptr) {
    hipStream_t st = c->stream;
    const int planes = pr ? 3 : 1;
    if (pr) h_image = pr->image;
    const std::vector<SkyPass> passes = sky_passes(c);
    const int n_pass = (int)passes.size();
    const int R = std::max(1, c->max_pairs), ks = std::max(2, c->max_k);
    const size_t npix2 = h_image ? (size_t)npixel * npixel : 0;
    const bool want_vis = vr && vr->vis;
    const int nbl = want_vis ? vr->nbl : 0, n_rblk = (R + SKYV_ROWS - 1) / SKYV_ROWS;
    const size_t vis_per_image = want_vis ? (size_t)(n_rblk + 1) * nbl * 2 : 0;  // partials + the combined chunk
    const int n_pblk = (R + SKYP_ROWS - 1) / SKYP_ROWS;
    const size_t pol_per_image = pr ? (size_t)n_pass * 3 * R + (size_t)n_pblk * 6 : 0;  // the polarization list + the Stokes partials
    const size_t per_t = sizeof(double) * ((size_t)nb * nnu * ((size_t)n_pass * 4 * R + planes * npix2 + vis_per_image + pol_per_image) +
                                           (size_t)nnu * nbl * 2);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>(nt, ((size_t)256 << 20) / per_t));
    if (const char* e = vag_hook("VAG_SKY_CHUNK_T")) chunk = std::max(1, std::min(nt, std::atoi(e)));
    const size_t G_max = (size_t)nb * nnu * chunk;
    if (c->d_skyterms.ensure(sizeof(double) * (size_t)n_pass * (pr ? 7 : 4) * G_max * R)) return VAG_E_HIP;
    if (h_image && c->d_skyimg.ensure(sizeof(double) * G_max * planes * npix2)) return VAG_E_HIP;
    if (want_vis && c->d_skyvis.ensure(sizeof(double) * G_max * vis_per_image)) return VAG_E_HIP;
    if (want_vis && c->d_skyuv.ensure(sizeof(double) * (size_t)nnu * chunk * nbl * 2)) return VAG_E_HIP;
    const size_t n_bins = (size_t)nb * nnu * nt;
    if (c->d_skymom.ensure(sizeof(double) * n_bins * 7)) return VAG_E_HIP;
    double* d_mom = c->d_skymom.as<double>();
    double* d_out = d_mom + n_bins * 6;
    double* d_pol = pr ? c->d_skyterms.as<double>() + (size_t)n_pass * 4 * G_max * R : nullptr;  // behind the largest chunk's term list
    double *d_spec = nullptr, *d_stokes = nullptr, *d_pout = nullptr;
    if (pr) {
        if (c->d_skypol.ensure(sizeof(double) * (size_t)n_pblk * G_max * 6)) return VAG_E_HIP;
        if (c->d_skystokes.ensure(sizeof(double) * ((size_t)nb * 4 + n_bins * 6))) return VAG_E_HIP;
        d_spec = c->d_skystokes.as<double>();
        d_stokes = d_spec + (size_t)nb * 4;
        d_pout = d_stokes + n_bins * 3;
        HIPCHK(hipMemcpyAsync(d_spec, pr->spec, sizeof(double) * (size_t)nb * 4, hipMemcpyHostToDevice, st));
    }
    int rc = VAG_OK;
    for (int t0 = 0; t0 < nt && rc == VAG_OK; t0 += chunk) {
        const int n = std::min(chunk, nt - t0);
        const size_t G = (size_t)nb * nnu * n;
        rc = sky_terms_stage(c, d_params, nb, t0, n, nnu, passes, R, ks, d_pol);
        if (rc) break;
        SkyImgArgs b{};
        b.meta = c->d_meta.as<VagGridMeta>();
        b.phi = c->d_phi.as<double>();
        b.terms = c->d_skyterms.as<double>();
        b.n_pass = n_pass;
        b.nnu = nnu;
        b.nt = n;
        b.R = R;
        b.n_az = n_az;
        b.nt_all = nt;
        b.t0 = t0;
        b.fov = h_image ? fov : 0.0;
        b.npixel = h_image ? npixel : 1;
        b.image = c->d_skyimg.as<double>();
        b.image_chunk = 1;
        b.extra_planes = planes - 1;
        b.moments = h_moments ? d_mom : nullptr;
        b.outside = h_outside ? d_out : nullptr;
        if (h_image) {
            const int tiles = (npixel + SKY_TILE - 1) / SKY_TILE;
            hipLaunchKernelGGL(vag_sky_deposit_kernel, dim3(tiles * tiles, (unsigned)G), dim3(64), 0, st, b);
            HIPCHK(hipGetLastError());
        }
        if (b.moments || b.outside) {
            hipLaunchKernelGGL(vag_sky_moments_kernel, dim3((unsigned)G), dim3(64), 0, st, b);
            HIPCHK(hipGetLastError());
        }
        if (pr) {
            SkyPolArgs pa = sky_pol_args(c, passes, nnu, n, R, n_az, nt, t0, d_pol, d_spec);
            pa.fov = pr->outside ? fov : 0.0;
            pa.npixel = pr->outside ? npixel : 1;
            pa.sin_2pa = std::sin(2 * pr->pa);
            pa.cos_2pa = std::cos(2 * pr->pa);
            pa.stokes = pr->stokes ? d_stokes : nullptr;
            pa.outside = pr->outside ? d_pout : nullptr;
            if (pa.stokes || pa.outside) {
                rc = sky_stokes_stage(c, pa, G, n_pblk);
                if (rc) break;
            }
            if (h_image) {
                const int tiles = (npixel + SKY_TILE - 1) / SKY_TILE;
                hipLaunchKernelGGL(vag_sky_stokes_deposit_kernel, dim3(tiles * tiles, (unsigned)G, 2), dim3(64), 0, st, b, pa);
                HIPCHK(hipGetLastError());
            }
        }
        if (h_image) {  // [nb * nnu][n][planes][npixel^2] -> its place in [nb * nnu][nt][planes][npixel^2]
            const size_t img = sizeof(double) * planes * npix2;
            HIPCHK(hipMemcpy2DAsync(h_image + (size_t)t0 * planes * npix2, nt * img, c->d_skyimg.p, n * img, n * img, (size_t)nb * nnu,
                                    hipMemcpyDeviceToHost, st));
        }
        if (want_vis) {
            const size_t row = sizeof(double) * n * nbl;  // this chunk's baselines: [nnu][t0 : t0 + n][nbl] -> [nnu][n][nbl]
            double* d_u = c->d_skyuv.as<double>();
            double* d_v = d_u + (size_t)nnu * n * nbl;
            HIPCHK(hipMemcpy2DAsync(d_u, row, vr->u + (size_t)t0 * nbl, sizeof(double) * nt * nbl, row, nnu, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpy2DAsync(d_v, row, vr->v + (size_t)t0 * nbl, sizeof(double) * nt * nbl, row, nnu, hipMemcpyHostToDevice, st));
            SkyVisArgs va{};
            va.meta = b.meta;
            va.phi = b.phi;
            va.terms = b.terms;
            va.u = d_u;
            va.v = d_v;
            va.n_pass = n_pass;
            va.nnu = nnu;
            va.nt = n;
            va.R = R;
            va.n_az = n_az;
            va.nbl = nbl;
            va.sin_pa = std::sin(vr->pa);
            va.cos_pa = std::cos(vr->pa);
            va.partial = c->d_skyvis.as<double>();
            double* d_vis = va.partial + (size_t)n_rblk * G * nbl * 2;
            const int n_blb = (nbl + 63) / 64;
            hipLaunchKernelGGL(vag_sky_visibility_kernel, dim3((unsigned)(G * n_blb), (unsigned)n_rblk), dim3(64), 0, st, va);
            HIPCHK(hipGetLastError());
            const size_t n_vis = G * nbl;
            hipLaunchKernelGGL(vag_sky_visibility_combine, dim3((unsigned)((n_vis + 255) / 256)), dim3(256), 0, st, b.meta, va.partial,
                               (int)G, nnu, n, nbl, d_vis);
            HIPCHK(hipGetLastError());
            // [nb * nnu][n][nbl][2] -> its place in [nb * nnu][nt][nbl][2]
            HIPCHK(hipMemcpy2DAsync(vr->vis + (size_t)t0 * nbl * 2, sizeof(double) * nt * nbl * 2, d_vis, 2 * row, 2 * row, (size_t)nb * nnu,
                                    hipMemcpyDeviceToHost, st));
        }
    }
    if (rc) return rc;
    if (h_moments) HIPCHK(hipMemcpyAsync(h_moments, d_mom, sizeof(double) * n_bins * 6, hipMemcpyDeviceToHost, st));
    if (h_outside) HIPCHK(hipMemcpyAsync(h_outside, d_out, sizeof(double) * n_bins, hipMemcpyDeviceToHost, st));
    if (pr && pr->stokes) HIPCHK(hipMemcpyAsync(pr->stokes, d_stokes, sizeof(double) * n_bins * 3, hipMemcpyDeviceToHost, st));
    if (pr && pr->outside) HIPCHK(hipMemcpyAsync(pr->outside, d_pout, sizeof(double) * n_bins * 3, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return VAG_OK;
}

static void (*centroid_kernel(int mode, bool spread))(SkyCenArgs) {  // vag_sky_centroid_kernel<mode, spread>: 3 photon sources x 2
    switch (mode) {
        case FLUX_SSC: return spread ? vag_sky_centroid_kernel<FLUX_SSC, true> : vag_sky_centroid_kernel<FLUX_SSC, false>;
        case FLUX_SYN_IC: return spread ? vag_sky_centroid_kernel<FLUX_SYN_IC, true> : vag_sky_centroid_kernel<FLUX_SYN_IC, false>;
        default: return spread ? vag_sky_centroid_kernel<FLUX_SYN, true> : vag_sky_centroid_kernel<FLUX_SYN, false>;
    }
}

// Exact sky moments of the whole batch (vag_sky_centroid_kernel); model stages already run, d_lg2t / d_lg2nu prepared.  The passes
// are sky_request's, each writing its row-block partials into its own slice; the combine reads the slices in that fixed order.  The
// time axis is cut into chunks whose partials stay within 256 MB (VAG_SKY_CHUNK_T: a test's chunk length).  d_moments
// [nb][nnu][nt][6] on the device.
int centroid_request(vag_ctx* c, const vag_model_params* d_params, int nb, int nt, int nnu, double* d_moments) {
    hipStream_t st = c->stream;
    struct SkyPass {
        int e, pass;
    };
    std::vector<SkyPass> passes;
    const int n_em = (c->batch_flags & VAG_FLAG_RVS) ? 2 : 1;
    for (int e = 0; e < n_em; ++e) {
        passes.push_back({e, 0});
        if (c->batch_flags & (e == 0 ? VAG_FLAG_SSC : VAG_FLAG_RVS_SSC)) passes.push_back({e, 1});
    }
    const int n_pass = (int)passes.size();
    const int n_blk = std::max(1, (c->max_pairs + SKYC_ROWS - 1) / SKYC_ROWS);
    const size_t per_t = sizeof(double) * (size_t)n_pass * nb * nnu * n_blk * 6;
    int chunk = (int)std::max<size_t>(1, std::min<size_t>(nt, ((size_t)256 << 20) / per_t));
    if (const char* e = vag_hook("VAG_SKY_CHUNK_T")) chunk = std::max(1, std::min(nt, std::atoi(e)));
    if (c->d_skycen.ensure(per_t * chunk)) return VAG_E_HIP;
    const bool spreading = (c->batch_flags & VAG_FLAG_SPREADING) != 0;
    int rc = VAG_OK;
    for (int t0 = 0; t0 < nt && rc == VAG_OK; t0 += chunk) {
        const int n = std::min(chunk, nt - t0);
        for (int q = 0; q < n_pass && rc == VAG_OK; ++q) {
            select_emitter(c, passes[q].e, d_params);
            SkyCenArgs a{};
            bind_batch(a, c, c->cur_params);
            bind_layout(a, c);
            a.phi = c->d_phi.as<double>();
            a.lg2_t_obs = c->d_lg2t.as<double>() + t0;
            a.lg2_nu_obs = c->d_lg2nu.as<double>();
            a.nt = n;
            a.nnu = nnu;
            a.n_blk = n_blk;
            a.partial = c->d_skycen.as<double>() + (size_t)q * nb * nnu * n * n_blk * 6;
            const int mode = passes[q].pass == 1 ? FLUX_SSC : (c->cur_ssc ? FLUX_SYN_IC : FLUX_SYN);
            auto rows = [&]() -> int {
                StageScope ps(c, mode == FLUX_SSC ? PS_SSC_FLUX : PS_SYNC_FLUX);
                a.ichdr = c->d_ichdr.as<double>();  // (behind the table build, which may reallocate them)
                a.icpool = c->d_icpool.as<double>();
                a.ic_status = c->d_icstatus.as<int>();
                hipLaunchKernelGGL(centroid_kernel(mode, spreading), dim3((n_blk + SKYC_WAVES - 1) / SKYC_WAVES, nb),
                                   dim3(SKYC_ROWS * SKYC_WAVES), 0, st, a);
                HIPCHK(hipGetLastError());
                return VAG_OK;
            };
            if (mode == FLUX_SSC) {  // the tables clamped to the requested frequencies exactly as a grid call clamps them
                rc = ssc_attempts(c, nb, [&](bool rebuild) {
                    const int rb = build_ssc_tables(c, c->cur_params, nb, c->d_lg2nu.as<double>(), nnu, rebuild);
                    return rb ? rb : rows();
                });
            } else {
                rc = rows();
            }
        }
        select_emitter(c, 0, d_params);
        if (rc) break;
        const int G = nb * nnu * n;
        hipLaunchKernelGGL(vag_sky_centroid_combine, dim3((G + 255) / 256), dim3(256), 0, st, c->d_meta.as<VagGridMeta>(),
                           c->d_skycen.as<double>(), n_pass, nb, nnu, n, n_blk, nt, t0, d_moments);
        HIPCHK(hipGetLastError());
    }
    return rc;
}

// One visibility group of a likelihood call (vag_sky_vis_chi2_kernel); model stages already run on the group's epochs, d_lg2t /
// d_lg2nu prepared.  The epochs are cut into chunks whose term list stays within 256 MB (VAG_SKY_CHUNK_T: a test's chunk length);
// every (walker, visibility block) partial is written once, by the chunk of its epoch, so the cut does not change a bit.
// d_vispart [nb][n_blk][2] afterwards.
int vis_chi2_request(vag_ctx* c, const vag_model_params* d_params, int nb, const vag_visibility_obs& o, const VisLayout& lay,
                     SkyVisFitArgs va) {
    hipStream_t st = c->stream;
    const std::vector<SkyPass> passes = sky_passes(c);
    const int n_pass = (int)passes.size(), nt = o.n_epochs;
    const int R = std::max(1, c->max_pairs), ks = std::max(2, c->max_k);
    const size_t per_t = sizeof(double) * (size_t)nb * n_pass * 4 * R;
    int chunk = (int)std::max<size_t>(1, std::min<size_t>(nt, ((size_t)256 << 20) / per_t));
    if (const char* e = vag_hook("VAG_SKY_CHUNK_T")) chunk = std::max(1, std::min(nt, std::atoi(e)));
    if (c->d_skyterms.ensure(per_t * chunk)) return VAG_E_HIP;
    const int n_blk_all = lay.epoch_blk[nt];
    if (c->d_vispart.ensure(sizeof(double) * 2 * (size_t)nb * n_blk_all)) return VAG_E_HIP;
    va.meta = c->d_meta.as<VagGridMeta>();
    va.phi = c->d_phi.as<double>();
    va.obs = c->vis.d.as<double>() + lay.obs_off + vis_cols(o).six;
    va.blocks = c->d_visblk.as<int>() + 3 * (size_t)lay.blk_off;
    va.n_vis = o.n_vis;
    va.n_blk_all = n_blk_all;
    va.n_pass = n_pass;
    va.R = R;
    va.n_az = o.n_az > 0 ? o.n_az : 1024;
    va.kind = o.kind;
    va.partial = c->d_vispart.as<double>();
    for (int t0 = 0; t0 < nt; t0 += chunk) {
        const int n = std::min(chunk, nt - t0);
        const int rc = sky_terms_stage(c, d_params, nb, t0, n, 1, passes, R, ks);
        if (rc) return rc;
        va.terms = c->d_skyterms.as<double>();
        va.t0 = t0;
        va.nt = n;
        va.blk0 = lay.epoch_blk[t0];
        va.n_blk = lay.epoch_blk[t0 + n] - va.blk0;
        if ((size_t)nb * va.n_blk > 0x7fffffffull) return set_err(VAG_E_CAPACITY, "visibility group: too many (walker, visibility block) pairs");
        hipLaunchKernelGGL(vag_sky_vis_chi2_kernel, dim3((unsigned)((size_t)nb * va.n_blk)), dim3(64), 0, st, va);
        HIPCHK(hipGetLastError());
    }
    return VAG_OK;
}

// One polarization group of a likelihood call; model stages already run on the group's epochs, d_lg2t / d_lg2nu prepared, the walkers'
// spec [nb][4] on the device.  The polarized terms stage and the Stokes kernels of sky_request, unchanged, without the turn by 2 pa:
// jet-frame I, Q, U into d_stokes [nb][nt][3], the bits of vag_sky_polarization_batch at pa = 0.  The epochs are cut into chunks
// whose term, polarization and partial lists stay within 256 MB (VAG_SKY_CHUNK_T: a test's chunk length); an epoch's sums do not
// depend on the cut.
int pol_stokes_request(vag_ctx* c, const vag_model_params* d_params, int nb, int nt, int n_az, const double* d_spec, double* d_stokes) {
    const std::vector<SkyPass> passes = sky_passes(c);
    const int n_pass = (int)passes.size();
    const int R = std::max(1, c->max_pairs), ks = std::max(2, c->max_k);
    const int n_pblk = (R + SKYP_ROWS - 1) / SKYP_ROWS;
    const size_t per_t = sizeof(double) * (size_t)nb * ((size_t)n_pass * 7 * R + (size_t)n_pblk * 6);
    int chunk = (int)std::max<size_t>(1, std::min<size_t>(nt, ((size_t)256 << 20) / per_t));
    if (const char* e = vag_hook("VAG_SKY_CHUNK_T")) chunk = std::max(1, std::min(nt, std::atoi(e)));
    const size_t G_max = (size_t)nb * chunk;
    if (G_max > 0x7fffffffull) return set_err(VAG_E_CAPACITY, "polarization group: too many (walker, epoch) pairs");
    if (c->d_skyterms.ensure(sizeof(double) * (size_t)n_pass * 7 * G_max * R)) return VAG_E_HIP;
    if (c->d_skypol.ensure(sizeof(double) * (size_t)n_pblk * G_max * 6)) return VAG_E_HIP;
    double* d_pol = c->d_skyterms.as<double>() + (size_t)n_pass * 4 * G_max * R;  // behind the largest chunk's term list
    for (int t0 = 0; t0 < nt; t0 += chunk) {
        const int n = std::min(chunk, nt - t0);
        int rc = sky_terms_stage(c, d_params, nb, t0, n, 1, passes, R, ks, d_pol);
        if (rc) return rc;
        SkyPolArgs pa = sky_pol_args(c, passes, 1, n, R, n_az, nt, t0, d_pol, d_spec);
        pa.sin_2pa = 0.0;
        pa.cos_2pa = 1.0;
        pa.stokes = d_stokes;
        rc = sky_stokes_stage(c, pa, (size_t)nb * n, n_pblk);
        if (rc) return rc;
    }
    return VAG_OK;
}

// Fixed-order sum of the workgroup partials of a series request.  A workgroup is 64 points x 4 block groups: group g adds the
// partial blocks b = g, g + 4, ... with four loads in flight, then the four group sums are added in order -- the same
// result run to run, and the walk over up to a few hundred blocks is no longer one dependent load after another
// (63 us per 128-walker call before).
__global__ void __launch_bounds__(256)
vag_series_reduce_kernel(const vag_model_params* __restrict__ params, const VagGridMeta* __restrict__ meta,
                         const double* __restrict__ partial, int max_blocks, int pairs_per_block, int n,
                         double* __restrict__ out, int parts /* partial sums per block of rows */,
                         int* __restrict__ work_counter = nullptr /* of the persistent launch before this one: back to zero */) {
    __shared__ double s_part[4][64];
    const int m = blockIdx.y;
    if (work_counter && blockIdx.x == 0 && m == 0 && threadIdx.x == 0) *work_counter = 0;
    const VagGridMeta M = meta[m];
    const vag_model_params P = params[m];
    const int nblk = (M.status == 0) ? (M.n_theta * M.n_phi_eff + pairs_per_block - 1) / pairs_per_block * parts : 0;
    const double d_L = P.lumi_dist * U_CM;
    const double norm = (1 + P.z) / (d_L * d_L);
    const double* src = partial + (size_t)m * max_blocks * n;
    const int g = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int s = blockIdx.x * 64 + lane;
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (s < n) {
        int b = g;
        for (; b + 12 < nblk; b += 16) {
            a0 += src[(size_t)b * n + s];
            a1 += src[(size_t)(b + 4) * n + s];
            a2 += src[(size_t)(b + 8) * n + s];
            a3 += src[(size_t)(b + 12) * n + s];
        }
        for (; b < nblk; b += 4) a0 += src[(size_t)b * n + s];
    }
    s_part[g][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (g == 0 && s < n) {
        const double v = (s_part[0][lane] + s_part[1][lane]) + (s_part[2][lane] + s_part[3][lane]);
        out[(size_t)m * n + s] = (M.status == 0) ? (v * norm) / U_FLUX_DEN_CGS : NAN;
    }
}

// vag_flux_fit_rows_kernel<mode, bands, spread, tally>: the 13 variants fit_rows_plan can give
static SeriesKernel fit_rows_kernel(const FitRowsVariant& v) {
    constexpr auto key = [](int mode, int bands, bool spread, bool tally = false) {
        return mode | (bands == 8 ? 4 : 0) | (spread ? 8 : 0) | (tally ? 16 : 0);
    };
    switch (key(v.mode, v.bands, v.spread, v.tally)) {
        case key(FLUX_SYN, 4, false): return vag_flux_fit_rows_kernel<FLUX_SYN, 4>;
        case key(FLUX_SYN, 8, false): return vag_flux_fit_rows_kernel<FLUX_SYN, 8>;
        case key(FLUX_SYN, 4, true): return vag_flux_fit_rows_kernel<FLUX_SYN, 4, true>;
        case key(FLUX_SYN, 8, true): return vag_flux_fit_rows_kernel<FLUX_SYN, 8, true>;
        case key(FLUX_SYN_IC, 4, false): return vag_flux_fit_rows_kernel<FLUX_SYN_IC, 4>;
        case key(FLUX_SYN_IC, 8, false): return vag_flux_fit_rows_kernel<FLUX_SYN_IC, 8>;
        case key(FLUX_SYN_IC, 4, true): return vag_flux_fit_rows_kernel<FLUX_SYN_IC, 4, true>;
        case key(FLUX_SYN_IC, 8, true): return vag_flux_fit_rows_kernel<FLUX_SYN_IC, 8, true>;
        case key(FLUX_SSC, 4, false): return vag_flux_fit_rows_kernel<FLUX_SSC, 4>;
        case key(FLUX_SSC, 8, false): return vag_flux_fit_rows_kernel<FLUX_SSC, 8>;
        case key(FLUX_SSC, 4, true): return vag_flux_fit_rows_kernel<FLUX_SSC, 4, true>;
        case key(FLUX_SSC, 8, true): return vag_flux_fit_rows_kernel<FLUX_SSC, 8, true>;
        case key(FLUX_SYN, 4, false, true): return vag_flux_fit_rows_kernel<FLUX_SYN, 4, false, true>;
    }
    return nullptr;
}

// vag_flux_series_kernel<mode, spread, points per lane, grid>: the 15 variants series_plan can give
static SeriesKernel series_kernel(const SeriesVariant& v) {
    constexpr int N = SERIES_MAX_SLOTS;
    constexpr auto key = [](int mode, bool spread, int slots, bool grid = false) {
        return mode | (spread ? 4 : 0) | (slots == 1 ? 8 : 0) | (grid ? 16 : 0);
    };
    switch (key(v.mode, v.spread, v.slots, v.grid)) {
        case key(FLUX_SYN, false, 1): return vag_flux_series_kernel<FLUX_SYN, false, 1>;
        case key(FLUX_SYN, false, N): return vag_flux_series_kernel<FLUX_SYN, false, N>;
        case key(FLUX_SYN, true, 1): return vag_flux_series_kernel<FLUX_SYN, true, 1>;
        case key(FLUX_SYN, true, N): return vag_flux_series_kernel<FLUX_SYN, true, N>;
        case key(FLUX_SYN_IC, false, 1): return vag_flux_series_kernel<FLUX_SYN_IC, false, 1>;
        case key(FLUX_SYN_IC, false, N): return vag_flux_series_kernel<FLUX_SYN_IC, false, N>;
        case key(FLUX_SYN_IC, true, 1): return vag_flux_series_kernel<FLUX_SYN_IC, true, 1>;
        case key(FLUX_SYN_IC, true, N): return vag_flux_series_kernel<FLUX_SYN_IC, true, N>;
        case key(FLUX_SSC, false, 1): return vag_flux_series_kernel<FLUX_SSC, false, 1>;
        case key(FLUX_SSC, false, N): return vag_flux_series_kernel<FLUX_SSC, false, N>;
        case key(FLUX_SSC, true, 1): return vag_flux_series_kernel<FLUX_SSC, true, 1>;
        case key(FLUX_SSC, true, N): return vag_flux_series_kernel<FLUX_SSC, true, N>;
        case key(FLUX_SYN, false, N, true): return vag_flux_series_kernel<FLUX_SYN, false, N, true>;
        case key(FLUX_SYN_IC, false, N, true): return vag_flux_series_kernel<FLUX_SYN_IC, false, N, true>;
        case key(FLUX_SSC, false, N, true): return vag_flux_series_kernel<FLUX_SSC, false, N, true>;
    }
    return nullptr;
}

int run_flux_series(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, const double* d_lg2nu,
                    int n, double* d_out, int mode, int n_bands, int grid_nt) {
    hipStream_t st = c->stream;
    StageScope ps(c, mode == FLUX_SSC ? PS_SSC_FLUX : PS_SYNC_FLUX);
    if (n > SERIES_THREADS * SERIES_MAX_SLOTS)
        return set_err(VAG_E_CAPACITY, "series length %d exceeds %d", n, SERIES_THREADS * SERIES_MAX_SLOTS);
    const FluxBatch batch = flux_batch(c, nb);
    const FluxHooks hooks = flux_hooks();
    const bool debug = vag_hook("VAG_DEBUG_LAUNCH") != nullptr;
    SeriesArgs a{};
    bind_batch(a, c, d_params);
    bind_layout(a, c);
    a.lg2_t_obs = d_lg2t;
    a.lg2_nu_obs = d_lg2nu;
    a.n = n;
    a.band_idx = c->d_bandidx.as<int>();
    a.band_first = c->d_bandidx.as<int>() + FITROWS_MAX_POINTS;
    // A fit's shape (plain synchrotron, <= 512 points in a few bands): the row-per-lane kernel (vag_fit_rows.h)
    if (fit_rows_takes(hooks, mode, grid_nt, n, n_bands)) {
        const FitRowsPlan p = fit_rows_plan(batch, hooks, mode, n_bands);
        if (c->d_partial.ensure(sizeof(double) * (size_t)nb * p.max_blocks * FITROWS_SEGS * n)) return VAG_E_HIP;
        a.pairs_per_block = FITROWS_ROWS;
        a.max_blocks = p.max_blocks;
        a.max_chunks = p.max_blocks * FITROWS_SEGS;  // one partial sum per (block of 64 rows, lattice segment)
        a.chunk = FITROWS_ROWS;
        a.partial = c->d_partial.as<double>();
        a.n_bands = n_bands;
        // (+=: a call with several series passes or chunks reports all of them; the plan is reset by the model stage of the call)
        const long long upper_evals = 2 * c->total_pairs * (long long)n, upper_interps = c->total_pairs * (long long)n;
        c->plan.spec_evals += upper_evals;
        c->plan.interps += upper_interps;
        c->plan.flux_blocks = p.max_blocks * nb;
        c->plan.pairs_per_block = FITROWS_ROWS;
        if (c->n_rows > 0) {
            a.grid_nt = p.waves_per_block;
            a.nb = nb;
            a.work = work_counters(c);
            const size_t lds = fit_rows_lds_bytes(n);
            const SeriesKernel kernel = fit_rows_kernel(p.v);
            if (!kernel) return set_err(VAG_E_INVALID, "no fit rows kernel for mode %d", mode);
            if (debug)
                std::fprintf(stderr, "[vag] fit rows launch: mode %d n=%d bands=%d blocks=%lld waves/block=%d spreading=%d lds=%zu B\n", mode, n,
                             n_bands, p.blocks, p.waves_per_block, (int)batch.spreading, lds);
            if (p.v.tally) {  // vag_ctx_count_work
                if (c->d_workcount.ensure(2 * sizeof(unsigned long long))) return VAG_E_HIP;
                HIPCHK(hipMemsetAsync(c->d_workcount.p, 0, 2 * sizeof(unsigned long long), st));
                a.tally = c->d_workcount.as<unsigned long long>();
            }
            hipLaunchKernelGGL(kernel, dim3(p.workgroups), dim3(SERIES_THREADS * FITROWS_WAVES), lds, st, a);
            HIPCHK(hipGetLastError());
            if (p.v.tally) {
                unsigned long long hcount[2] = {0, 0};
                HIPCHK(hipMemcpyAsync(hcount, c->d_workcount.p, sizeof hcount, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                c->plan.spec_evals += (long long)hcount[0] - upper_evals;  // the tallied counts replace this pass's upper bounds
                c->plan.interps += (long long)hcount[1] - upper_interps;
            }
        }
        HIPCHK(hipEventRecord(c->ev[4], st));
        hipLaunchKernelGGL(vag_series_reduce_kernel, dim3((n + 63) / 64, nb), dim3(256), 0, st, d_params, c->d_meta.as<VagGridMeta>(),
                           c->d_partial.as<double>(), p.max_blocks * FITROWS_SEGS, FITROWS_ROWS, n, d_out, FITROWS_SEGS, work_counters(c));
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(c->ev[5], st));
        return VAG_OK;
    }
    const SeriesPlan p = series_plan(batch, hooks, mode, n, n_bands, grid_nt);
    if (c->d_partial.ensure(sizeof(double) * (size_t)nb * p.max_chunks * n)) return VAG_E_HIP;
    const int ks = flux_ks(batch, hooks);
    // wavefronts per workgroup: four when their private rows fit next to the shared tables, else two or one
    auto lds_for = [&](int w) {
        return sizeof(double) * ((size_t)w * series_region_doubles(ks, mode == FLUX_SYN_IC, p.n_bands) + SP_LDS_DOUBLES + SERIES_MAX_BANDS);
    };
    // (the runtime's occupancy query decides what fits: two 80 KB workgroups do not share a CU's 160 KB.  The figure is the one of
    // <FLUX_SYN, false, 1> whatever variant is launched, as it was measured with)
    const void* const occ_fn = reinterpret_cast<const void*>(vag_flux_series_kernel<FLUX_SYN, false, 1>);
    auto occ_for = [&](int w) {
        const int wg = wg_per_cu(c, occ_fn, SERIES_THREADS * w, lds_for(w));
        return wg < 0 ? (int)((144 * 1024) / std::max<size_t>(lds_for(w), 1)) : wg;
    };
    int wg[3] = {-1, -1, -1};
    for (int i = 0; i < 3 && lds_for(1 << i) <= CU_LDS_BYTES; ++i) wg[i] = occ_for(1 << i);
    const int waves = series_waves(hooks, wg);
    const size_t lds = lds_for(waves);
    if (lds > CU_LDS_BYTES) return set_err(VAG_E_CAPACITY, "LDS request %zu B exceeds 160 KiB (n_t=%d)", lds, ks);
    const dim3 sgrid((p.max_blocks + waves - 1) / waves, nb), sblock(SERIES_THREADS * waves);
    if (debug)
        std::fprintf(stderr, "[vag] series launch: n=%d bands=%d max_k=%d rows/wave=%lld waves/wg=%d lds=%zu B grid=(%u,%u) wg/CU=%d\n", n,
                     p.n_bands, ks, p.ppb, waves, lds, sgrid.x, sgrid.y, wg_per_cu(c, occ_fn, SERIES_THREADS * waves, lds));
    a.n_bands = p.n_bands;
    a.grid_nt = grid_nt;
    a.chunk = p.chunk;
    a.pairs_per_block = (int)p.ppb;
    a.max_blocks = p.max_blocks;
    a.max_chunks = p.max_chunks;
    a.k_stride = ks;
    a.partial = c->d_partial.as<double>();
    c->plan.spec_evals = 2 * c->total_pairs * (long long)n;
    c->plan.interps = c->total_pairs * (long long)n;
    c->plan.flux_blocks = p.max_blocks * nb;
    c->plan.pairs_per_block = (int)p.ppb;
    if (c->n_rows > 0) {
        const SeriesKernel kernel = series_kernel(p.v);
        if (!kernel) return set_err(VAG_E_INVALID, "no series kernel for mode %d", mode);
        hipLaunchKernelGGL(kernel, sgrid, sblock, lds, st, a);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev[4], st));
    hipLaunchKernelGGL(vag_series_reduce_kernel, dim3((n + 63) / 64, nb), dim3(256), 0, st, d_params,
                       c->d_meta.as<VagGridMeta>(), c->d_partial.as<double>(), p.max_chunks, p.chunk, n, d_out, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[5], st));
    return VAG_OK;
}

// One chunk of a (t, nu) series for the batch.  d_out (optional) [nb][n] receives the sum of every enabled component in
// PyFlux::calc_total order; d_comp (optional) -> d_comp[i] != nullptr receives component i of {fwd.sync, fwd.ssc, rvs.sync,
// rvs.ssc} [nb][n], zeros when that component is disabled.
int series_chunk(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_lg2t, const double* d_lg2nu, int n,
                 const double* d_lg2nu_all, int n_all, double* d_out, int n_bands = 0, double* const* d_comp = nullptr) {
    const int n_em = (c->batch_flags & VAG_FLAG_RVS) ? 2 : 1;
    const size_t n_out = (size_t)nb * n;
    int rc = VAG_OK;
    bool first = true;
    for (int e = 0; e < 2 && rc == VAG_OK; ++e) {
        if (e < n_em) select_emitter(c, e, d_params);
        for (int pass = 0; pass < 2 && rc == VAG_OK; ++pass) {
            double* dst_comp = d_comp ? d_comp[2 * e + pass] : nullptr;
            const bool enabled = e < n_em && (pass == 0 || c->cur_ssc);
            if (!enabled) {
                if (dst_comp && hipMemsetAsync(dst_comp, 0, sizeof(double) * n_out, c->stream) != hipSuccess) rc = VAG_E_HIP;
                continue;
            }
            double* dst = dst_comp;
            if (!dst) {
                if (!d_out) continue;  // nobody wants this component
                if (first) {
                    dst = d_out;
                } else {
                    if (c->d_ssc.ensure(sizeof(double) * n_out)) {
                        rc = VAG_E_HIP;
                        break;
                    }
                    dst = c->d_ssc.as<double>();
                }
            }
            if (pass == 0) {
                rc = run_flux_series(c, c->cur_params, nb, d_lg2t, d_lg2nu, n, dst, c->cur_ssc ? FLUX_SYN_IC : FLUX_SYN, n_bands);
            } else {
                rc = ssc_attempts(c, nb, [&](bool rebuild) {
                    const int rb = build_ssc_tables(c, c->cur_params, nb, d_lg2nu_all, n_all, rebuild);
                    return rb ? rb : run_flux_series(c, c->cur_params, nb, d_lg2t, d_lg2nu, n, dst, FLUX_SSC, n_bands);
                });
            }
            if (rc) break;
            if (d_out) {
                if (first) {
                    if (dst != d_out) hipLaunchKernelGGL(vag_copy_kernel, dim3(256), dim3(256), 0, c->stream, d_out, dst, n_out);
                } else {
                    hipLaunchKernelGGL(vag_add_kernel, dim3(256), dim3(256), 0, c->stream, d_out, dst, n_out);
                }
                if (hipGetLastError() != hipSuccess) rc = VAG_E_HIP;
            }
            first = false;
        }
    }
    select_emitter(c, 0, d_params);
    return rc;
}

int collect_times(vag_ctx* c) {
    HIPCHK(hipEventSynchronize(c->ev[5]));
    float v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[0], c->ev[1]));
    c->times.grid_ms = v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[1], c->ev[2]));
    c->times.dynamics_ms = v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[2], c->ev[3]));
    c->times.cells_ms = v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[3], c->ev[4]));
    c->times.flux_ms = v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[4], c->ev[5]));
    c->times.reduce_ms = v;
    HIPCHK(hipEventElapsedTime(&v, c->ev[0], c->ev[5]));
    c->times.total_ms = v;
    return VAG_OK;
}

int prep_times(vag_ctx* c, const double* d_t, int nt, const double* d_nu, int nnu) {
    if (c->d_lg2t.ensure(sizeof(double) * nt)) return VAG_E_HIP;
    if (c->d_lg2nu.ensure(sizeof(double) * std::max(1, nnu))) return VAG_E_HIP;
    if (c->d_tminmax.ensure(sizeof(double) * 2)) return VAG_E_HIP;
    hipLaunchKernelGGL(vag_prep_kernel, dim3(1), dim3(256), 0, c->stream, d_t, nt, d_nu, nnu, c->d_lg2t.as<double>(),
                       c->d_lg2nu.as<double>(), c->d_tminmax.as<double>());
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

int check_host_inputs(const vag_model_params* params, int nb, const double* t, int nt) {
    if (!params || !t) return set_err(VAG_E_INVALID, "null model or time array");
    if (nb <= 0) return set_err(VAG_E_INVALID, "batch must be non-empty");
    if (nt <= 0) return set_err(VAG_E_INVALID, "time array must be non-empty");
    for (int i = 0; i < nt; ++i)
        if (!(t[i] > 0) || !std::isfinite(t[i])) return set_err(VAG_E_INVALID, "times must be positive and finite");
    for (int i = 1; i < nt; ++i)
        if (t[i] < t[i - 1]) return set_err(VAG_E_INVALID, "time array must be in ascending order");
    for (int m = 0; m < nb; ++m) {
        const char* msg = validate_msg(&params[m]);
        if (msg) return set_err(VAG_E_INVALID, "model %d: %s", m, msg);
    }
    return VAG_OK;
}

// the batch's grid results on the host, copied only when someone needs more than the plan's totals
int fetch_meta(vag_ctx* c) {
    if (c->meta_on_host) return VAG_OK;
    if (c->h_meta.ensure(sizeof(VagGridMeta) * (size_t)c->nb)) return VAG_E_HIP;
    HIPCHK(hipMemcpyAsync(c->h_meta.p, c->d_meta.p, sizeof(VagGridMeta) * (size_t)c->nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->meta_on_host = true;
    return VAG_OK;
}

// End of a call that was planned from the previous call's summary (run_model_stages, spec): read this batch's own summary and
// verify the assumptions.  VAG_RETRY: a capacity was exceeded (the device then skipped every model) or the flags / kernel class
// differ -- the caller repeats the call on the waiting path, which also refreshes the hint.
constexpr int VAG_RETRY = 1;
int finish_speculation(vag_ctx* c) {
    if (!c->spec_pending) return VAG_OK;
    c->spec_pending = false;
    VagDevPlan* hp = c->h_plan.as<VagDevPlan>();
    if (int rcw = wait_plan(c)) return rcw;  // the grid stage finished long ago: the later stages keep running behind this check
    const PlanVerdict v = plan_ahead_verdict(*hp, c->hint, c->spec_cap_k, c->spec_margin_k);
    if (v.repeat) {
        const int flags = plan_flags(*hp), hflags = plan_flags(c->hint);
        if (vag_hook("VAG_DEBUG_SPEC"))
            std::fprintf(stderr, "[vag] planned-ahead call repeated: overflow %d mixed %d flags %d/%d dyn %d/%d rows %d cells %lld max_k %d (cap %d) max_pairs %d; hint rows %d cells %lld max_k %d max_pairs %d\n",
                         hp->overflow, hp->flags_mixed, flags, hflags, hp->dyn_class, c->hint.dyn_class, hp->rows, (long long)hp->cells,
                         hp->max_k, c->spec_cap_k, hp->max_pairs, c->hint.rows, (long long)c->hint.cells, c->hint.max_k, c->hint.max_pairs);
        c->spec_margin_k = v.margin_k;  // (more where the lattice outgrew its head room)
        c->hint_valid = false;
        return VAG_RETRY;
    }
    c->hint = *hp;
    c->hint_valid = hp->n_ok > 0;
    c->n_ok = hp->n_ok;
    c->plan.n_models_ok = hp->n_ok;
    c->plan.n_rows = hp->rows;
    c->plan.n_cells = hp->cells;
    c->plan.total_pairs = hp->pairs;
    c->plan.eat_cells = hp->eat;
    c->plan.n_models_invalid = hp->n_invalid;
    c->plan.n_models_capacity = hp->n_capacity;
    return VAG_OK;
}

int check_status(vag_ctx* c, int nb) {
    const int rf = read_row_failures(c);
    if (rf) return rf;
    if (c->plan.n_rows_failed > 0)
        return set_err(VAG_E_NUMERIC, "%d ODE row(s): no acceptable step size after 500 rejections", c->plan.n_rows_failed);
    if (c->plan.n_models_capacity == 0) return VAG_OK;
    if (fetch_meta(c)) return VAG_E_HIP;
    const VagGridMeta* hm = c->h_meta.as<VagGridMeta>();
    for (int m = 0; m < nb; ++m)
        if (hm[m].status == VAG_E_CAPACITY)
            return set_err(VAG_E_CAPACITY, "model %d: adaptive grid exceeds engine limits (theta %d, phi %d, time %d)", m,
                           VAG_HUGE_THETA, VAG_HUGE_PHI, VAG_MAX_TIME);
    return VAG_OK;
}

}  // namespace

// ---- batches whose models carry different Radiation / shock flags (ssc, kn, rvs, spreading, magnetar, non-axisymmetric) ----
// One launch sequence serves one flag set (the flags pick kernels and passes).  The reference evaluates any mix of models
// side by side (samplers.py:59-91), so a mixed batch handed over the host-pointer API is split by flags, every group runs as
// its own batch -- same entry point, same arithmetic as if the caller had split it --, and the groups' rows are put back in
// place.  OutRows: one output array of `stride` doubles per model (NULL: not requested).  ins: per-model input arrays of the same
// form, gathered per group and handed to the call behind the outputs.
struct OutRows {
    double* p;
    size_t stride;
};
static bool uniform_flags(const vag_model_params* params, int nb) {
    for (int m = 1; m < nb; ++m)
        if (params[m].flags != params[0].flags) return false;
    return true;
}
template <class Call>
static int run_flag_groups(const vag_model_params* params, int nb, const std::vector<OutRows>& outs, Call call,
                           const std::vector<OutRows>& ins = {}) {
    for (const std::vector<int>& idx : group_by_flags(nb, [&](int m) { return params[m].flags; })) {
        const int ng = (int)idx.size();
        std::vector<vag_model_params> gp(ng);
        for (int i = 0; i < ng; ++i) gp[i] = params[idx[i]];
        std::vector<std::vector<double>> bufs(outs.size() + ins.size());
        std::vector<double*> ptrs(outs.size() + ins.size(), nullptr);
        for (size_t q = 0; q < outs.size(); ++q)
            if (outs[q].p) {
                bufs[q].resize((size_t)ng * outs[q].stride);
                ptrs[q] = bufs[q].data();
            }
        for (size_t q = 0; q < ins.size(); ++q)
            if (ins[q].p) {
                std::vector<double>& buf = bufs[outs.size() + q];
                buf.resize((size_t)ng * ins[q].stride);
                for (int i = 0; i < ng; ++i)
                    std::memcpy(buf.data() + (size_t)i * ins[q].stride, ins[q].p + (size_t)idx[i] * ins[q].stride, sizeof(double) * ins[q].stride);
                ptrs[outs.size() + q] = buf.data();
            }
        const int rc = call(gp.data(), ng, ptrs);
        if (rc) return rc;
        for (size_t q = 0; q < outs.size(); ++q)
            if (outs[q].p)
                for (int i = 0; i < ng; ++i)
                    std::memcpy(outs[q].p + (size_t)idx[i] * outs[q].stride, bufs[q].data() + (size_t)i * outs[q].stride,
                                sizeof(double) * outs[q].stride);
    }
    return VAG_OK;
}

// ---- the frame of the host-pointer model requests: a batch of models, times and (but for a band) frequencies on the host, outputs
//      of one row per model.  An entry point keeps its own argument checks and its body -- the request it makes on device pointers;
//      everything between the two is here. ----
struct DevRows {  // where outs[first .. first + count) live on the device: in `buf`, [count][nb][stride] (sized for all of them)
    DevBuf vag_ctx::*buf;
    int first, count;
};
struct HostRequest {
    const vag_model_params* params;
    int nb;
    const double* t;
    int nt;
    const double* nu;
    int nnu;
    std::vector<OutRows> outs;  // the caller's output arrays (p NULL: not requested)
    std::vector<DevRows> dev;   // their device side; none: the body delivers to outs itself (sky_request copies in chunks)
    bool times = true;          // collect_times behind the call (the flux events it reads are not recorded by the sky passes)
    std::vector<OutRows> ins = {};  // per-model input arrays, gathered per group where the batch is split by flags
    bool has_nu = true;  // false: the body makes its own frequencies (a band), d_nu is not touched here and nu is not looked at
};
// check_host_inputs -> a batch of mixed flags: every flag set as a request of its own, same body -> the device -> d_params, d_t, d_nu
// and the output buffers, the uploads -> body(request, d_params, d_outs) -> the downloads -> the wait -> collect_times -> check_status.
// d_outs[i]: the device array of outs[i], NULL where it is not requested or has no device side.
template <class Body>
static int host_request(vag_ctx* c, const HostRequest& r, Body body) {
    int rc = check_host_inputs(r.params, r.nb, r.t, r.nt);
    if (rc) return rc;
    if (!uniform_flags(r.params, r.nb))
        return run_flag_groups(r.params, r.nb, r.outs, [&](const vag_model_params* gp, int ng, const std::vector<double*>& o) {
            HostRequest g = r;
            g.params = gp, g.nb = ng;
            for (size_t i = 0; i < g.outs.size(); ++i) g.outs[i].p = o[i];
            for (size_t i = 0; i < g.ins.size(); ++i) g.ins[i].p = o[g.outs.size() + i];
            return host_request(c, g, body);
        }, r.ins);
    HIPCHK(hipSetDevice(c->device));
    const size_t nb = (size_t)r.nb;
    if (c->d_params.ensure(sizeof(vag_model_params) * nb)) return VAG_E_HIP;
    if (c->d_t.ensure(sizeof(double) * r.nt)) return VAG_E_HIP;
    if (r.has_nu && c->d_nu.ensure(sizeof(double) * r.nnu)) return VAG_E_HIP;
    for (const DevRows& d : r.dev)
        if ((c->*d.buf).ensure(sizeof(double) * d.count * nb * r.outs[d.first].stride)) return VAG_E_HIP;
    HIPCHK(hipMemcpyAsync(c->d_params.p, r.params, sizeof(vag_model_params) * nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_t.p, r.t, sizeof(double) * r.nt, hipMemcpyHostToDevice, c->stream));
    if (r.has_nu) HIPCHK(hipMemcpyAsync(c->d_nu.p, r.nu, sizeof(double) * r.nnu, hipMemcpyHostToDevice, c->stream));
    std::vector<double*> d_outs(r.outs.size(), nullptr);
    for (const DevRows& d : r.dev)
        for (int i = 0; i < d.count; ++i)
            if (r.outs[d.first + i].p) d_outs[d.first + i] = (c->*d.buf).as<double>() + i * nb * r.outs[d.first].stride;
    rc = body(r, c->d_params.as<vag_model_params>(), d_outs.data());
    if (rc) return rc;
    if (!r.dev.empty()) {
        for (size_t i = 0; i < d_outs.size(); ++i)
            if (d_outs[i]) HIPCHK(hipMemcpyAsync(r.outs[i].p, d_outs[i], sizeof(double) * nb * r.outs[i].stride, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (r.times) (void)collect_times(c);
    return check_status(c, r.nb);
}

extern "C" {

int vag_last_stage_times(vag_ctx* c, vag_stage_times* out) {
    ApiLock api_lock(c);
    if (!c || !out) return set_err(VAG_E_INVALID, "null context or output");
    // measured with HIP events recorded on the context stream around each kernel of the last batch call
    const int rc = collect_times(c);
    *out = c->times;
    return rc;
}

}  // extern "C"

// ---- device-resident batches with mixed Radiation / shock flags (samplers.py:59-91 evaluates any mix of models side by side) ----
__global__ void vag_flags_kernel(const vag_model_params* __restrict__ params, int nb, int* __restrict__ flags) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < nb) flags[m] = params[m].flags;
}
__global__ void vag_gather_params_kernel(const vag_model_params* __restrict__ params, const int* __restrict__ perm, int nb,
                                         vag_model_params* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) out[i] = params[perm[i]];
}
__global__ void vag_scatter_rows_kernel(const double* __restrict__ src, const int* __restrict__ perm, int nb, size_t stride,
                                        double* __restrict__ dst) {
    // gridDim.y is capped (65535): a workgroup row takes every gridDim.y-th model
    for (int i = blockIdx.y; i < nb; i += gridDim.y) {
        const double* s = src + (size_t)i * stride;
        double* d = dst + (size_t)perm[i] * stride;
        for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < stride; q += (size_t)gridDim.x * blockDim.x) d[q] = s[q];
    }
}

// A batch the grid pass refused for its mixed flags: sort the models by flags (stable: the flags travel to the host, 4 bytes per
// model, the permutation comes back), run every group as a batch of its own on the gathered parameters -- each model then comes
// out bitwise as in a call of its own group -- and scatter the rows back into the caller's order.  `body(d_params, n, d_out)` is
// the single-flag path of the entry point.
template <class Body>
static int flux_dev_by_flags(vag_ctx* c, const vag_model_params* d_params, int nb, size_t stride, double* d_out, Body body) {
    if (c->d_mix_flags.ensure(sizeof(int) * (size_t)nb) || c->d_mix_perm.ensure(sizeof(int) * (size_t)nb) ||
        c->d_mix_params.ensure(sizeof(vag_model_params) * (size_t)nb) || c->d_mix_out.ensure(sizeof(double) * (size_t)nb * stride))
        return VAG_E_HIP;
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(vag_flags_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, d_params, nb, c->d_mix_flags.as<int>());
    HIPCHK(hipGetLastError());
    std::vector<int> flags(nb), perm;
    HIPCHK(hipMemcpyAsync(flags.data(), c->d_mix_flags.p, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const std::vector<std::vector<int>> groups = group_by_flags(nb, [&](int m) { return flags[m]; });
    perm.reserve(nb);
    for (const auto& g : groups) perm.insert(perm.end(), g.begin(), g.end());
    HIPCHK(hipMemcpyAsync(c->d_mix_perm.p, perm.data(), sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // perm is a local: the copy must have left it
    hipLaunchKernelGGL(vag_gather_params_kernel, dim3((nb + 127) / 128), dim3(128), 0, st, d_params, c->d_mix_perm.as<int>(), nb,
                       c->d_mix_params.as<vag_model_params>());
    HIPCHK(hipGetLastError());
    size_t off = 0;
    int n_ok = 0, n_inv = 0, n_cap = 0;
    for (const auto& g : groups) {
        const int ng = (int)g.size();
        const int rc = body(c->d_mix_params.as<vag_model_params>() + off, ng, c->d_mix_out.as<double>() + off * stride);
        if (rc) return rc;
        n_ok += c->plan.n_models_ok, n_inv += c->plan.n_models_invalid, n_cap += c->plan.n_models_capacity;
        off += (size_t)ng;
    }
    c->plan.n_models_ok = n_ok, c->plan.n_models_invalid = n_inv, c->plan.n_models_capacity = n_cap;  // the batch's, not the last group's
    const unsigned gx = (unsigned)std::min<size_t>((stride + 255) / 256, 64);
    hipLaunchKernelGGL(vag_scatter_rows_kernel, dim3(gx, (unsigned)std::min(nb, 65535)), dim3(256), 0, st, c->d_mix_out.as<double>(),
                       c->d_mix_perm.as<int>(), nb, stride, d_out);
    HIPCHK(hipGetLastError());
    c->hint_valid = false;  // the hint is the LAST GROUP's plan: the next mixed batch of this size must not be planned from it
    return VAG_OK;
}

// A call on device pointers under the plan-ahead protocol.  attempt(may_plan): the model stages with that switch, then the request.
// The first attempt may be planned from the previous call's summary (run_model_stages) and is verified at its end; where the plan
// did not hold, or the planned call failed (an error while planning from stale sizes is not the caller's), the call is repeated
// once on the waiting path.  A failure that is not a planned call's -- prep_times ahead of the stages, or any failure of the second
// attempt -- is returned as it is: spec_pending is set by run_model_stages alone, which clears it first, and no path leaves it set
// between calls.  what: "grid" / "series", for the VAG_DEBUG_SPEC line.
template <class Attempt>
static int plan_ahead_attempts(vag_ctx* c, const char* what, Attempt attempt) {
    int rc = VAG_OK;
    for (int n = 0; n < 2; ++n) {
        rc = attempt(n == 0 && !c->count_work);
        if (rc) {
            if (!c->spec_pending) return rc;
            c->spec_pending = false;
            c->hint_valid = false;
            if (vag_hook("VAG_DEBUG_SPEC")) std::fprintf(stderr, "[vag] planned-ahead %s call failed (%d: %s): repeating\n", what, rc, g_err.c_str());
            continue;
        }
        rc = finish_speculation(c);
        if (rc != VAG_RETRY) break;
    }
    return rc;
}

extern "C" {

static int grid_dev_body(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_t, int nt, const double* d_nu, int nnu,
                         double* d_out) {
    return plan_ahead_attempts(c, "grid", [&](bool may_plan) {
        int rc = prep_times(c, d_t, nt, d_nu, nnu);
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, nb, false, may_plan);
        return rc ? rc : grid_request_chunked(c, d_params, nb, nt, nnu, nullptr, d_out, nullptr);
    });
}

int vag_flux_density_grid_batch_dev(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_t, int nt,
                                    const double* d_nu, int nnu, double* d_out) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!d_params || !d_t || !d_nu || !d_out) return set_err(VAG_E_INVALID, "null device pointer");
    if (nb <= 0 || nt <= 0 || nnu <= 0) return set_err(VAG_E_INVALID, "empty batch, time or frequency array");
    HIPCHK(hipSetDevice(c->device));
    c->mixed_flags_seen = false;
    int rc = grid_dev_body(c, d_params, nb, d_t, nt, d_nu, nnu, d_out);
    if (rc == VAG_E_UNSUPPORTED && c->mixed_flags_seen)
        rc = flux_dev_by_flags(c, d_params, nb, (size_t)nnu * nt, d_out, [&](const vag_model_params* gp, int ng, double* o) {
            return grid_dev_body(c, gp, ng, d_t, nt, d_nu, nnu, o);
        });
    return rc;
}

static int upload_series_bands(vag_ctx* c, const double* nu, int n);

// The whole (t, nu) series already in c->d_lg2t / c->d_lg2nu (prep_times) -> d_out[nb][n], the sum of every enabled
// component.  Longer series than one launch holds (exposure sampling, large data sets) go through in chunks of sorted
// points on the same model grid.
// d4 (in place of d_out): the components {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} apart, [nb][n] each, NULL entries skipped.
static int series_request(vag_ctx* c, const vag_model_params* d_params, int nb, int n, double* d_out, int n_bands,
                          double* const* d4 = nullptr) {
    const int chunk = SERIES_THREADS * SERIES_MAX_SLOTS;
    const double *lg2t = c->d_lg2t.as<double>(), *lg2nu = c->d_lg2nu.as<double>();
    if (n <= chunk) return series_chunk(c, d_params, nb, lg2t, lg2nu, n, lg2nu, n, d_out, n_bands, d4);
    double* const total[1] = {d_out};
    double* const* dst = d4 ? d4 : total;
    const int n_dst = d4 ? 4 : 1;
    const size_t rows = (size_t)nb * chunk;  // of one output: the scratch holds one set for the total, four for the components
    DevBuf& tmp = c->d_chunk;  // grow-only context scratch: the stream orders its reuse
    if (tmp.ensure(sizeof(double) * n_dst * rows)) return VAG_E_HIP;
    int rc = VAG_OK;
    for (int s0 = 0; s0 < n && rc == VAG_OK; s0 += chunk) {  // chunks of sorted points on the same grid
        const int m = std::min(chunk, n - s0);
        double* part[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < n_dst; ++i) part[i] = dst[i] ? tmp.as<double>() + i * rows : nullptr;
        rc = series_chunk(c, d_params, nb, lg2t + s0, lg2nu + s0, m, lg2nu, n, d4 ? nullptr : part[0], 0, d4 ? part : nullptr);
        for (int i = 0; i < n_dst && rc == VAG_OK; ++i)
            if (dst[i] && hipMemcpy2DAsync(dst[i] + s0, sizeof(double) * n, part[i], sizeof(double) * m, sizeof(double) * m, (size_t)nb,
                                           hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                rc = VAG_E_HIP;
    }
    return rc;
}

static int series_dev_body(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_t, const double* d_nu, int n,
                           double* d_out, int n_bands) {
    return plan_ahead_attempts(c, "series", [&](bool may_plan) {
        int rc = prep_times(c, d_t, n, d_nu, n);  // the grid sees the extrema of ALL requested times
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, nb, false, may_plan);
        return rc ? rc : series_request(c, d_params, nb, n, d_out, n_bands);
    });
}

int vag_flux_density_batch_dev(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_t,
                               const double* d_nu, int n, double* d_out) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!d_params || !d_t || !d_nu || !d_out) return set_err(VAG_E_INVALID, "null device pointer");
    if (nb <= 0 || n <= 0) return set_err(VAG_E_INVALID, "empty batch or data array");
    HIPCHK(hipSetDevice(c->device));
    const int n_bands = c->pending_bands;  // only the host-pointer wrapper below knows the frequencies
    c->pending_bands = 0;
    c->mixed_flags_seen = false;
    int rc = series_dev_body(c, d_params, nb, d_t, d_nu, n, d_out, n_bands);
    if (rc == VAG_E_UNSUPPORTED && c->mixed_flags_seen)
        rc = flux_dev_by_flags(c, d_params, nb, (size_t)n, d_out, [&](const vag_model_params* gp, int ng, double* o) {
            return series_dev_body(c, gp, ng, d_t, d_nu, n, o, n_bands);
        });
    return rc;
}

int vag_flux_density_grid_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt,
                                const double* nu, int nnu, double* out) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !out) return set_err(VAG_E_INVALID, "null frequency or output array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    const HostRequest r{params, nb, t, nt, nu, nnu, {{out, (size_t)nnu * nt}}, {{&vag_ctx::d_out, 0, 1}}};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d) {
        return vag_flux_density_grid_batch_dev(c, d_params, q.nb, c->d_t.as<double>(), nt, c->d_nu.as<double>(), nnu, d[0]);
    });
}

// out4 = {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc}; NULL entries are skipped
static int grid_components_impl(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu,
                                int nnu, double* const* out4) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    const size_t st = (size_t)nnu * nt;
    const HostRequest r{params, nb, t, nt, nu, nnu, {{out4[0], st}, {out4[1], st}, {out4[2], st}, {out4[3], st}}, {{&vag_ctx::d_comp, 0, 4}}};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d4) {
        int rc = prep_times(c, c->d_t.as<double>(), nt, c->d_nu.as<double>(), nnu);
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, q.nb, false);
        return rc ? rc : grid_request_chunked(c, d_params, q.nb, nt, nnu, nullptr, nullptr, d4);
    });
}

int vag_flux_density_grid_components_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt,
                                           const double* nu, int nnu, double* out_sync, double* out_ssc) {
    ApiLock api_lock(c);
    double* out4[4] = {out_sync, out_ssc, nullptr, nullptr};
    return grid_components_impl(c, params, nb, t, nt, nu, nnu, out4);
}

int vag_flux_density_grid_components4_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt,
                                            const double* nu, int nnu, double* const* out4) {
    ApiLock api_lock(c);
    if (!out4) return set_err(VAG_E_INVALID, "out4 must not be null");
    if (!nu) return set_err(VAG_E_INVALID, "null frequency array");
    return grid_components_impl(c, params, nb, t, nt, nu, nnu, out4);
}

// Model.sky_image / Model.sky_moments over a batch (vag_sky.h; the definition is the engine's own)
static int sky_impl(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu, int n_az,
                    double fov, int npixel, double* image, double* outside, double* moments, const SkyVisReq* vr = nullptr,
                    const SkyPolReq* pr = nullptr) {
    const size_t st = (size_t)nnu * nt;
    const SkyPolReq none{};
    const SkyPolReq& P = pr ? *pr : none;
    // (no device side: sky_request copies its outputs in chunks; no collect_times: the flux events it reads are not recorded by the sky passes)
    const HostRequest r{params, nb, t, nt, nu, nnu,
                        {{image, st * npixel * npixel}, {outside, st}, {moments, st * 6}, {vr ? vr->vis : nullptr, vr ? st * vr->nbl * 2 : 0},
                         {P.stokes, st * 3}, {P.image, st * 3 * npixel * npixel}, {P.outside, st * 3}},
                        {}, false, {{const_cast<double*>(P.spec), 4}}};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const*) {
        const std::vector<OutRows>& o = q.outs;
        SkyVisReq gv{};
        if (vr) gv = *vr, gv.vis = o[3].p;
        const SkyPolReq gpol{q.ins[0].p, P.pa, o[4].p, o[5].p, o[6].p};
        int rc = prep_times(c, c->d_t.as<double>(), nt, c->d_nu.as<double>(), nnu);
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, q.nb, false);
        return rc ? rc : sky_request(c, d_params, q.nb, nt, nnu, n_az, fov, npixel, o[0].p, o[1].p, o[2].p, vr ? &gv : nullptr, pr ? &gpol : nullptr);
    });
}

int vag_sky_image_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                        double fov, int npixel, int n_az, double* image, double* outside) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !image) return set_err(VAG_E_INVALID, "null frequency or image array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    if (!(std::isfinite(fov) && fov > 0)) return set_err(VAG_E_INVALID, "fov must be positive and finite");
    if (npixel < 1 || npixel > 4096) return set_err(VAG_E_INVALID, "npixel must be in [1, 4096]");
    if (n_az <= 0) n_az = 4 * npixel;
    return sky_impl(c, params, nb, t, nt, nu, nnu, n_az, fov, npixel, image, outside, nullptr);
}

int vag_sky_moments_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                          int n_az, double* moments) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !moments) return set_err(VAG_E_INVALID, "null frequency or moments array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    if (n_az <= 0) n_az = 256;
    return sky_impl(c, params, nb, t, nt, nu, nnu, n_az, 0.0, 1, nullptr, nullptr, moments);
}

int vag_sky_visibility_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                             const double* u, const double* v, int nbl, double pa, int n_az, double* vis) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !u || !v || !vis) return set_err(VAG_E_INVALID, "null frequency, baseline or visibility array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    if (nbl <= 0 || nbl > VAG_SKY_MAX_BASELINES)
        return set_err(VAG_E_INVALID, "nbl must be in [1, %d], got %d", VAG_SKY_MAX_BASELINES, nbl);
    if (nt > 0) {  // (bad times: check_host_inputs)
        const size_t n = (size_t)nnu * nt * nbl;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(u[i]) || !std::isfinite(v[i])) return set_err(VAG_E_INVALID, "baselines u, v must be finite");
    }
    if (!std::isfinite(pa)) return set_err(VAG_E_INVALID, "pa must be finite");
    if (n_az <= 0) n_az = 1024;
    const SkyVisReq vr{u, v, nbl, pa, vis};
    return sky_impl(c, params, nb, t, nt, nu, nnu, n_az, 0.0, 1, nullptr, nullptr, nullptr, &vr);
}

// Model.sky_polarization / Model.sky_stokes_image over a batch ("Polarization").  spec [nb][4]: b - 1 of the forward
// and reverse shock, then their Pi_max (pi_max < 0: (p + 1) / (p + 7/3) with that emitter's own p).
static int pol_spec(const vag_model_params* params, int nb, const vag_pol_spec* pol, std::vector<double>& spec) {
    if (!params || nb <= 0) return VAG_OK;  // (check_host_inputs reports it)
    spec.resize((size_t)nb * 4);
    for (int m = 0; m < nb; ++m)
        for (int e = 0; e < 2; ++e) {
            const double b = pol[m].b[e], p = e == 0 ? params[m].p : params[m].rvs_p;
            double pm = pol[m].pi_max[e];
            if (!(std::isfinite(b) && b >= 0)) return set_err(VAG_E_INVALID, "model %d: pol.b[%d] must be finite and >= 0", m, e);
            if (std::isnan(pm) || pm > 1) return set_err(VAG_E_INVALID, "model %d: pol.pi_max[%d] must be <= 1 (< 0: from p)", m, e);
            if (pm < 0) pm = (p + 1) / (p + 7.0 / 3.0);
            spec[4 * (size_t)m + e] = b - 1;
            spec[4 * (size_t)m + 2 + e] = pm;
        }
    return VAG_OK;
}

int vag_sky_polarization_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                               const vag_pol_spec* pol, double pa, int n_az, double* out) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !pol || !out) return set_err(VAG_E_INVALID, "null frequency, polarization spec or output array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    if (!std::isfinite(pa)) return set_err(VAG_E_INVALID, "pa must be finite");
    std::vector<double> spec;
    if (int rc = pol_spec(params, nb, pol, spec)) return rc;
    if (n_az <= 0) n_az = 256;
    const SkyPolReq pr{spec.data(), pa, out, nullptr, nullptr};
    return sky_impl(c, params, nb, t, nt, nu, nnu, n_az, 0.0, 1, nullptr, nullptr, nullptr, nullptr, &pr);
}

int vag_sky_stokes_image_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                               const vag_pol_spec* pol, double fov, int npixel, int n_az, double* image, double* outside) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !pol || !image) return set_err(VAG_E_INVALID, "null frequency, polarization spec or image array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    if (!(std::isfinite(fov) && fov > 0)) return set_err(VAG_E_INVALID, "fov must be positive and finite");
    if (npixel < 1 || npixel > 4096) return set_err(VAG_E_INVALID, "npixel must be in [1, 4096]");
    std::vector<double> spec;
    if (int rc = pol_spec(params, nb, pol, spec)) return rc;
    if (n_az <= 0) n_az = 4 * npixel;
    const SkyPolReq pr{spec.data(), 0.0, nullptr, image, outside};
    return sky_impl(c, params, nb, t, nt, nu, nnu, n_az, fov, npixel, nullptr, nullptr, nullptr, nullptr, &pr);
}

// Test-facing probe of the device math (vag_debug_math.h): not on any product path, synchronous, its own buffers.
int vag_debug_device_math(vag_ctx* c, int fn, const double* in, int n, double* out) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    const int n_in = math_n_in(fn), n_out = math_n_out(fn);
    if (n_in == 0) return set_err(VAG_E_INVALID, "unknown device routine %d", fn);
    if (!in || !out) return set_err(VAG_E_INVALID, "null input or output array");
    if (n <= 0) return set_err(VAG_E_INVALID, "n must be positive, got %d", n);
    if (math_is_wave(fn) && n % 64 != 0) return set_err(VAG_E_INVALID, "wave routine %d needs n %% 64 == 0, got %d", fn, n);
    if (fn == VAG_MATH_LDS_ADD)
        for (int i = 0; i < n; ++i)
            if (!(in[2 * (size_t)i] >= 0 && in[2 * (size_t)i] < 64 && in[2 * (size_t)i] == std::floor(in[2 * (size_t)i])))
                return set_err(VAG_E_INVALID, "point %d: lds_add_f64 slot must be an integer in [0, 64)", i);
    for (int i = 0; i < n; ++i)
        if (const char* why = math_point_error(fn, in + (size_t)i * n_in)) return set_err(VAG_E_INVALID, "device routine %d, point %d: %s", fn, i, why);
    HIPCHK(hipSetDevice(c->device));
    struct Bufs {
        DevBuf in, out, col;
        ~Bufs() {
            in.release();
            out.release();
            col.release();
        }
    } b;
    const size_t bytes_in = sizeof(double) * (size_t)n * n_in, bytes_out = sizeof(double) * (size_t)n * n_out;
    if (b.in.ensure(bytes_in) || b.out.ensure(bytes_out)) return VAG_E_HIP;
    if (fn == VAG_MATH_SYN_CELL && b.col.ensure(sizeof(double) * (size_t)n * VAG_NPAR)) return VAG_E_HIP;
    HIPCHK(hipMemcpyAsync(b.in.p, in, bytes_in, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vag_math_probe_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), MATH_PROBE_LDS, c->stream, fn, n,
                       b.in.as<double>(), b.out.as<double>(), c->d_sptab.as<double>(), b.col.as<double>(), c->d_knlut.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, b.out.p, bytes_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VAG_OK;
}

// Model.sky_moments(exact=True) over a batch: the n_az -> infinity limit of sky_impl's moments (vag_sky_centroid_kernel)
static int centroid_impl(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                         double* moments) {
    const HostRequest r{params, nb, t, nt, nu, nnu, {{moments, (size_t)nnu * nt * 6}}, {{&vag_ctx::d_skycmom, 0, 1}}, false};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d) {
        int rc = prep_times(c, c->d_t.as<double>(), nt, c->d_nu.as<double>(), nnu);
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, q.nb, false);
        return rc ? rc : centroid_request(c, d_params, q.nb, nt, nnu, d[0]);
    });
}

int vag_sky_centroid_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                           double* moments) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !moments) return set_err(VAG_E_INVALID, "null frequency or moments array");
    if (nnu <= 0) return set_err(VAG_E_INVALID, "frequency array must be non-empty");
    return centroid_impl(c, params, nb, t, nt, nu, nnu, moments);
}

int vag_flux_density_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, const double* nu, int n,
                           double* out) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!nu || !out) return set_err(VAG_E_INVALID, "null frequency or output array");
    const HostRequest r{params, nb, t, n, nu, n, {{out, (size_t)n}}, {{&vag_ctx::d_out, 0, 1}}};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d) {
        CallMode<int> bands(c->pending_bands, upload_series_bands(c, nu, n));  // (the device-pointer entry point does not see the frequencies)
        return vag_flux_density_batch_dev(c, d_params, q.nb, c->d_t.as<double>(), c->d_nu.as<double>(), n, d[0]);
    });
}

// Model.flux_density with its components apart (FluxDict.fwd / .rvs of a series, pymodel.cpp:373-389): out4[i] != NULL
// receives component i of {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} [nb][n]; disabled components come back as zeros.
int vag_flux_density_components4_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, const double* nu,
                                       int n, double* const* out4) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!out4) return set_err(VAG_E_INVALID, "out4 must not be null");
    if (!nu) return set_err(VAG_E_INVALID, "null frequency array");
    const size_t st = (size_t)n;
    const HostRequest r{params, nb, t, n, nu, n, {{out4[0], st}, {out4[1], st}, {out4[2], st}, {out4[3], st}}, {{&vag_ctx::d_comp, 0, 4}}};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d4) {
        const int n_bands = upload_series_bands(c, nu, n);
        int rc = prep_times(c, c->d_t.as<double>(), n, c->d_nu.as<double>(), n);  // the grid sees the extrema of ALL requested times
        if (rc == VAG_OK) rc = run_model_stages(c, d_params, q.nb, false);
        return rc ? rc : series_request(c, d_params, q.nb, n, nullptr, n_bands, d4);  // (a long series, exposure sampling: in chunks)
    });
}

// Band request with parameters and times already in HBM: nu = logspace(nu_min, nu_max, num_nu) nodes with Boole weights
// (Observer::flux, src/core/quadrature.h:153-196, pymodel.cpp:391-410), own grid from the request's own time range.
// d_total (optional) [nb][nt] receives the sum of the enabled components, d4 (optional) the components apart.
static int band_request_dev(vag_ctx* c, const vag_model_params* d_params, int nb, const double* d_t, int nt, double nu_min,
                            double nu_max, int num_nu, double* d_total, double* const* d4) {
    if (!(nu_min > 0)) return set_err(VAG_E_INVALID, "nu_min must be positive");
    if (!(nu_max > nu_min)) return set_err(VAG_E_INVALID, "nu_max must be greater than nu_min");
    if (num_nu < 2) return set_err(VAG_E_INVALID, "num_nu must be at least 2");
    if (num_nu > VAG_MAX_NU) return set_err(VAG_E_CAPACITY, "at most %d band frequencies", VAG_MAX_NU);
    // nu = xt::logspace(log10(nu_min Hz), log10(nu_max Hz), num_nu) in code units
    std::vector<double> nu_code(num_nu), nu_cgs(num_nu), w(num_nu, 0.0);
    {
        const double a = std::log10(nu_min * U_HZ), b = std::log10(nu_max * U_HZ);
        const double step = (b - a) / std::fmax(1.0, (double)(num_nu - 1));
        for (int i = 0; i < num_nu; ++i) {
            nu_code[i] = std::pow(10.0, (i == num_nu - 1) ? b : a + step * (double)i);
            nu_cgs[i] = nu_code[i] / U_HZ;
        }
        const int n = num_nu;
        const double h = std::log(nu_code[1] / nu_code[0]);
        const double cb = 2.0 * h / 45.0;
        int j = 0;
        for (; j + 4 < n; j += 4) {
            w[j] += cb * 7;
            w[j + 1] += cb * 32;
            w[j + 2] += cb * 12;
            w[j + 3] += cb * 32;
            w[j + 4] += cb * 7;
        }
        const int rem = n - 1 - j;
        if (rem == 3) {
            const double c38 = 3.0 * h / 8.0;
            w[j] += c38;
            w[j + 1] += c38 * 3;
            w[j + 2] += c38 * 3;
            w[j + 3] += c38;
        } else if (rem == 2) {
            const double c13 = h / 3.0;
            w[j] += c13;
            w[j + 1] += c13 * 4;
            w[j + 2] += c13;
        } else if (rem == 1) {
            w[j] += 0.5 * h;
            w[j + 1] += 0.5 * h;
        }
        for (int i = 0; i < n; ++i) w[i] *= nu_code[i];
    }
    if (c->d_nu.ensure(sizeof(double) * num_nu)) return VAG_E_HIP;
    if (c->d_bandw.ensure(sizeof(double) * num_nu)) return VAG_E_HIP;
    HIPCHK(hipMemcpyAsync(c->d_nu.p, nu_cgs.data(), sizeof(double) * num_nu, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_bandw.p, w.data(), sizeof(double) * num_nu, hipMemcpyHostToDevice, c->stream));
    int rc = prep_times(c, d_t, nt, c->d_nu.as<double>(), num_nu);
    if (rc) return rc;
    // the band nodes are exact code-unit values: overwrite log2(nu_cgs * Hz) with log2(nu_code) to avoid a round trip
    std::vector<double> lg2nu(num_nu);
    for (int i = 0; i < num_nu; ++i) lg2nu[i] = std::log2(nu_code[i]);
    HIPCHK(hipMemcpyAsync(c->d_lg2nu.p, lg2nu.data(), sizeof(double) * num_nu, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // the staging vectors above are stack-local
    rc = run_model_stages(c, d_params, nb, false);
    if (rc) return rc;
    return grid_request_chunked(c, d_params, nb, nt, num_nu, c->d_bandw.as<double>(), d_total, d4);
}

// Model.flux for a batch: out_total (optional) receives the sum of the enabled components, out4 (optional) the
// components {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} apart (NULL entries skipped).
static int flux_band_impl(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, double nu_min,
                          double nu_max, int num_nu, double* out_total, double* const* out4) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!out_total && !out4) return set_err(VAG_E_INVALID, "null output array");
    const size_t st = (size_t)nt;
    const HostRequest r{params, nb, t, nt, nullptr, 0,
                        {{out_total, st}, {out4 ? out4[0] : nullptr, st}, {out4 ? out4[1] : nullptr, st}, {out4 ? out4[2] : nullptr, st},
                         {out4 ? out4[3] : nullptr, st}},
                        {{&vag_ctx::d_out, 0, 1}, {&vag_ctx::d_comp, 1, 4}}, /* times */ true, /* ins */ {}, /* has_nu */ false};
    return host_request(c, r, [&](const HostRequest& q, const vag_model_params* d_params, double* const* d) {
        return band_request_dev(c, d_params, q.nb, c->d_t.as<double>(), nt, nu_min, nu_max, num_nu, d[0], out4 ? d + 1 : nullptr);
    });
}

int vag_flux_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, double nu_min,
                   double nu_max, int num_nu, double* out) {
    ApiLock api_lock(c);
    return flux_band_impl(c, params, nb, t, nt, nu_min, nu_max, num_nu, out, nullptr);
}

int vag_flux_components_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, double nu_min,
                              double nu_max, int num_nu, double* out_sync, double* out_ssc) {
    ApiLock api_lock(c);
    double* out4[4] = {out_sync, out_ssc, nullptr, nullptr};
    return flux_band_impl(c, params, nb, t, nt, nu_min, nu_max, num_nu, nullptr, out4);
}

int vag_flux_components4_batch(vag_ctx* c, const vag_model_params* params, int nb, const double* t, int nt, double nu_min,
                               double nu_max, int num_nu, double* const* out4) {
    ApiLock api_lock(c);
    if (!out4) return set_err(VAG_E_INVALID, "out4 must not be null");
    return flux_band_impl(c, params, nb, t, nt, nu_min, nu_max, num_nu, nullptr, out4);
}

// Distinct frequencies of a short series (n <= 64, at most 8 of them): uploads [band of point s | first point of band b]
// and returns the number of bands, 0 when the shared-node path does not apply.
static int upload_series_bands(vag_ctx* c, const double* nu, int n) {
    constexpr int MAXB = SERIES_MAX_BANDS;
    if (n <= 0 || n > FITROWS_MAX_POINTS) return 0;
    int buf[FITROWS_MAX_POINTS + MAXB] = {};
    double vals[MAXB];
    int nbands = 0;
    for (int s = 0; s < n; ++s) {
        int b = 0;
        while (b < nbands && vals[b] != nu[s]) ++b;
        if (b == nbands) {
            if (nbands == MAXB) return 0;
            vals[nbands] = nu[s];
            buf[FITROWS_MAX_POINTS + nbands] = s;
            ++nbands;
        }
        buf[s] = b;
    }
    if (2 * nbands > n) return 0;  // nothing to share
    if (c->h_bands_n == nbands && std::memcmp(c->h_bandbuf, buf, sizeof buf) == 0) return nbands;  // already resident
    if (c->d_bandidx.ensure(sizeof buf)) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;  // an earlier copy may still read h_bandbuf
    std::memcpy(c->h_bandbuf, buf, sizeof buf);
    c->h_bands_n = nbands;
    if (hipMemcpyAsync(c->d_bandidx.p, c->h_bandbuf, sizeof buf, hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        c->h_bands_n = -1;
        return 0;
    }
    return nbands;
}

// ---- the uploads of a request's spec blocks (layouts, scans and miss halves: vag_fit_request.h), in the order in which their
//      refusals surface.  A block hashed in place is scanned here, when its turn comes; one that fit_request_prepare has scanned and
//      staged has no miss half but the copy of its stage vector.  fit_only: the fit block alone (a sharded call). ----
static int upload_blocks(vag_ctx* c, FitRequest& r, bool fit_only = false) {
    hipStream_t st = c->stream;
    int rc = fit_scan(r.spec, r.ndim, fit_accepts(r), r.fit);
    if (!rc) rc = c->fit.upload(st, r.fit, [&] { return fit_rows(r.spec); }, [&](double* hp) { fit_fill(r.spec, r.fit, hp); });
    if (rc || fit_only) return rc;
    if (r.sky && !(rc = sky_scan(r.sky, r.slay)))  // (n_groups = 0: the fixed placement alone)
        rc = c->sky.upload(st, r.slay, [&] { return sky_rows(r.sky); }, [&](double* hp) { six_fill(r.sky, r.slay, hp); });
    if (!rc && r.vis && !(rc = vis_scan(r.vis, r.vkey))) {  // (its int32 blocks ride behind the doubles, to d_visblk)
        rc = c->vis.upload(st, r.vkey, [&] { return vis_rows(r.vis, r.vis_groups, r.vis_blocks); },
                           [&](double* hp) { vis_fill(r.vis, r.vis_groups, hp); }, &r.vis_blocks, &c->d_visblk);
        if (!rc && !r.vis_groups.empty()) c->vis_layout = std::move(r.vis_groups);  // (a miss: vis_rows has laid the groups out anew)
    }
    if (!rc && r.pol && !(rc = pol_scan(r.pol, r.play)))
        rc = c->pol.upload(st, r.play, [&] { return pol_rows(r.pol); }, [&](double* hp) { six_fill(r.pol, r.play, hp); });
    const struct { ResidentBlock* block; const void* spec; const BlockKey* key; const std::vector<double>* staged; } scanned[8] = {  // (spec null: not held)
        {&c->lim, r.lim, &r.llay, &r.lstage},       {&c->noise, r.noise, &r.nlay, &r.nstage},
        {&c->counts, r.counts, &r.clay, &r.cstage}, {&c->index, r.index, &r.ilay, &r.istage},
        {&c->fold, r.fold, &r.flay, &r.fstage},     {&c->tmpl, r.tmpl, &r.tlay, &r.tstage},
        {&c->cov, r.cov, &r.vlay, &r.vstage},       {&c->robust, r.robust, &r.rlay, &r.rstage}};
    for (const auto& s : scanned)
        if (!rc && s.spec)
            rc = s.block->upload(st, *s.key, [] { return VAG_OK; },
                                 [&](double* hp) { std::memcpy(hp, s.staged->data(), sizeof(double) * s.staged->size()); });
    return rc;
}

constexpr int COUNTS_PPB = 64;  // (theta, phi) pairs per flux workgroup of a counts pass (vag_ctx::ppb_pin)

static int loglike_passes(vag_ctx* c, const FitRequest& req, const double* d_theta, int nb, int ndim, double* d_out, bool try_spec) {
    const vag_fit_spec* spec = req.spec;
    const vag_sky_fit_spec* sky = req.sky;
    int rc = VAG_OK;
    const int n = spec->n_data;
    hipStream_t st = c->stream;
    if (c->d_params.ensure(sizeof(vag_model_params) * nb)) return VAG_E_HIP;
    if (c->d_valid.ensure(sizeof(int) * nb)) return VAG_E_HIP;
    if (c->d_chi2.ensure(sizeof(double) * 3 * (size_t)nb)) return VAG_E_HIP;  // [chi2 | A_V | ln prior]
    if (c->d_fitstat.ensure(sizeof(int) * 4)) return VAG_E_HIP;
    if (c->d_lg2t.ensure(sizeof(double) * std::max(n, 1))) return VAG_E_HIP;
    if (c->d_lg2nu.ensure(sizeof(double) * std::max(n, 1))) return VAG_E_HIP;
    if (c->d_tminmax.ensure(sizeof(double) * 2)) return VAG_E_HIP;
    double* d_chi2 = c->d_chi2.as<double>();
    double* d_av = d_chi2 + nb;
    double* d_lp = d_chi2 + 2 * (size_t)nb;
    const FitLayout& fl = req.fit;
    double* d = c->fit.d.as<double>();  // the point block: [t | nu | ln_flux | ln_err | weight | ext]
    const double *ln_flux = d + fl.ln_flux, *ln_err = d + fl.ln_err, *weight = d + fl.weight, *ext = d + fl.ext;
    const double* d_prior = d + fl.prior;
    vag_model_params* d_params = c->d_params.as<vag_model_params>();
    // evaluation order: by the costs of the previous call with this batch size (see vag_ctx::d_order)
    const bool can_order = nb >= 64 && nb <= 8192 && !vag_hook("VAG_NO_ORDER");
    const int* d_order = (can_order && c->order_nb == nb) ? c->d_order[c->order_cur].as<int>() : nullptr;
    c->last_order = d_order;  // (every pass sets it again; a call without a pass leaves no stale order to vag_fit_split_kernel)
    hipLaunchKernelGGL(vag_fit_front_kernel, dim3((nb + 127) / 128), dim3(128), 0, st, spec->base, d_theta, nb, ndim, d_prior,
                       spec->use_priors, spec->a_v_fixed, d_params, d_av, d_lp, c->d_fitstat.as<int>(), d, n, d + fl.nu,
                       c->d_lg2t.as<double>(), c->d_lg2nu.as<double>(), c->d_tminmax.as<double>(), d_order);
    HIPCHK(hipGetLastError());
    bool order_made = false;
    // once per call, from the first pass's grids: the order the NEXT call evaluates in -- made by the first back kernel that can be a
    // call's first (its wavefronts are one per evaluation slot: no launch of its own on the call's critical path since round 6)
    auto next_order = [&]() -> FitOrderOut {
        FitOrderOut o{c->d_cost_f.as<float>(), nb, nullptr};
        if (!can_order || order_made) return o;
        DevBuf& nxt = c->d_order[c->order_cur ^ 1];
        if (nxt.ensure(sizeof(int) * (size_t)nb)) return o;
        order_made = true;
        o.next_order = nxt.as<int>();
        return o;
    };
    const std::vector<PassItem> passes = fit_pass_list(req);  // the call's passes: position 0 is the first, the final one the last
    size_t pass = 0;
    int n_cap = 0, n_inv = 0;  // per-pass rejection counts: the call reports the worst pass
    // what the current pass's back kernel receives (built at its launch: the model stages may have moved the buffers); the SSC tables
    // of a pass report per-model failures in d_icstatus: in a fit they invalidate the walker, they do not raise
    auto fit_pass = [&]() -> FitPass {
        const bool ssc = (c->batch_flags & (VAG_FLAG_SSC | VAG_FLAG_RVS_SSC)) != 0;
        return {c->d_meta.as<VagGridMeta>(), c->d_row_status.as<int>(), c->d_row_off.as<int>(),
                (ssc && c->d_icstatus.p) ? c->d_icstatus.as<int>() : nullptr, d_chi2, c->d_valid.as<int>(), d_lp, pass == 0 ? 1 : 0,
                pass + 1 == passes.size() ? 1 : 0, d_out, c->d_fitstat.as<int>(), d_order};
    };
    auto begin_pass = [&] {  // before the pass's model request
        c->order_next = d_order != nullptr;
        c->last_order = d_order;
    };
    auto end_pass = [&]() -> int {  // behind the pass's back kernel
        HIPCHK(hipGetLastError());
        n_cap = std::max(n_cap, c->plan.n_models_capacity);
        n_inv = std::max(n_inv, c->plan.n_models_invalid);
        return VAG_OK;
    };
    // the back of a flux pass.  lim_off: where the pass's block of limit rows starts in lim.d, or -1 (no limit row: the kernel as it
    // was); noise_off, present: where the pass's group ids start in noise.d, or -1 (no grouped row: the kernels as they were), and
    // its groups; tmpl_off, tpresent: where the pass's template values start in tmpl.d, or -1 (no touched row: the kernels as they
    // were), and the templates that touch it; robust: the pass holds a detection row of a robust group (its rows are grouped:
    // noise_off >= 0), else the kernels as they were
    auto back = [&](const double* flux, int npts, const double* lnf, const double* lne, const double* w, const double* ext,
                    long lim_off, long noise_off, unsigned present, long tmpl_off, unsigned tpresent, bool robust) -> int {
        const double* lb = lim_off >= 0 ? c->lim.d.as<double>() + lim_off : nullptr;  // [limit | sigma | kind]
        const LimCols lcol = lim_cols(npts);
        const int* lk = lb ? reinterpret_cast<const int*>(lb + lcol.kind) : nullptr;
        const double* ls = lb ? lb + lcol.sigma : nullptr;
        if (robust && noise_off >= 0) {
            const double* nz = c->noise.d.as<double>();
            const double* tp = tmpl_off >= 0 ? c->tmpl.d.as<double>() : nullptr;  // [amp_fixed 8 | the passes' values], or no template here
            hipLaunchKernelGGL(vag_fit_back_robust_kernel, dim3(nb), dim3(64), 0, st, flux, npts, lnf, lne, w, ext, d_av, fit_pass(),
                               next_order(), lk, lb, ls, d_theta, ndim, d_prior, nz, reinterpret_cast<const int*>(nz + noise_off), present,
                               tp ? tp + tmpl_off : nullptr, tp ? req.tlay.n_templates : 0, tp ? tpresent : 0u, tp, req.tlay.ext_mask,
                               c->robust.d.as<double>(), req.rlay.mask);
        } else if (tmpl_off >= 0) {
            const double* nz = noise_off >= 0 ? c->noise.d.as<double>() : nullptr;
            const double* tp = c->tmpl.d.as<double>();  // [amp_fixed 8 | the passes' values]
            hipLaunchKernelGGL(vag_fit_back_tmpl_kernel, dim3(nb), dim3(64), 0, st, flux, npts, lnf, lne, w, ext, d_av, fit_pass(),
                               next_order(), lk, lb, ls, d_theta, ndim, d_prior, nz, nz ? reinterpret_cast<const int*>(nz + noise_off) : nullptr,
                               nz ? present : 0u, tp + tmpl_off, req.tlay.n_templates, tpresent, tp, req.tlay.ext_mask);
        } else if (noise_off >= 0) {
            const double* nz = c->noise.d.as<double>();
            hipLaunchKernelGGL(vag_fit_back_noise_kernel, dim3(nb), dim3(64), 0, st, flux, npts, lnf, lne, w, ext, d_av, fit_pass(),
                               next_order(), lk, lb, ls, d_theta, ndim, d_prior, nz, reinterpret_cast<const int*>(nz + noise_off), present);
        } else {
            hipLaunchKernelGGL(lb ? vag_fit_back_kernel<true> : vag_fit_back_kernel<false>, dim3(nb), dim3(64), 0, st, flux, npts, lnf,
                               lne, w, ext, d_av, fit_pass(), next_order(), lk, lb, ls);
        }
        return end_pass();
    };
    // the front half of a series-group pass (index, fold, cov groups): the group's np points, whose times and frequencies lie at d_t
    // and d_nu of its resident block, through the model stages and one series request.  nu_pts: the points' frequencies on the host
    // for the shared-node test of a short series, or null for none.  Leaves the fluxes in d_series_flux (room_for_flux(np) has made
    // the room) or hands the failure back.
    auto series_group_flux = [&](const double* d_t, const double* d_nu, size_t np, const double* nu_pts) -> int {
        int r = prep_times(c, d_t, (int)np, d_nu, (int)np);
        begin_pass();
        if (r == VAG_OK) r = run_model_stages(c, d_params, nb, false);
        if (r == VAG_OK)  // (in chunks above 512 points)
            r = series_request(c, d_params, nb, (int)np, c->d_series_flux.as<double>(), nu_pts ? upload_series_bands(c, nu_pts, (int)np) : 0);
        return r;
    };
    // its counterpart for a centroid, visibility or polarization group, whose block is [nu | t ...] at ds with n times at ds + t_at:
    // the times behind the one frequency, through the model stages; the group's own request follows
    auto sky_group_stages = [&](const double* ds, size_t t_at, int nt) -> int {
        int r = prep_times(c, ds + t_at, nt, ds, 1);
        begin_pass();
        if (r == VAG_OK) r = run_model_stages(c, d_params, nb, false);
        return r;
    };
    // room in d_series_flux for a flux pass of np points per walker (never less than the point rows'); not 0: no memory
    auto room_for_flux = [&](size_t np) { return c->d_series_flux.ensure(sizeof(double) * (size_t)nb * std::max(np, (size_t)std::max(n, 1))); };
    for (; pass < passes.size() && rc == VAG_OK; ++pass) {  // (a failure ends the passes; what follows the loop still runs)
        const int g = passes[pass].group;
        switch (passes[pass].kind) {
        case PassKind::Point: {  // point data: one (t, nu) series per walker (fitter.py:510-522)
            if (room_for_flux(n)) return VAG_E_HIP;
            begin_pass();
            rc = run_model_stages(c, d_params, nb, false, try_spec);
            if (rc == VAG_OK) rc = series_request(c, d_params, nb, n, c->d_series_flux.as<double>(), upload_series_bands(c, spec->nu, n));
            if (rc == VAG_OK)
                rc = back(c->d_series_flux.as<double>(), n, ln_flux, ln_err, weight, spec->ext_kernel ? ext : nullptr,
                          req.lim ? req.llay.point : -1, req.noise ? req.nlay.point : -1, req.noise ? req.nlay.point_present : 0u,
                          req.tmpl ? req.tlay.point : -1, req.tmpl ? req.tlay.point_present : 0u, req.robust && req.rlay.point);
            if (rc == VAG_OK) {
                rc = finish_speculation(c);  // before a band group's own grid pass reuses the plan buffers
                n_cap = std::max(n_cap, c->plan.n_models_capacity);
                n_inv = std::max(n_inv, c->plan.n_models_invalid);
            } else if (c->spec_pending) {  // an error while planning from stale sizes: repeat the call on the waiting path
                if (vag_hook("VAG_DEBUG_SPEC"))
                    std::fprintf(stderr, "[vag] planned-ahead likelihood call failed (%d: %s): repeating\n", rc, g_err.c_str());
                c->spec_pending = false;
                c->hint_valid = false;
                rc = VAG_RETRY;
            }
        } break;
        case PassKind::Band: {  // band-integrated groups: one Model.flux request each (fitter.py:524-531)
            const vag_band_obs& bd = spec->bands[g];
            if (room_for_flux(bd.n)) return VAG_E_HIP;
            const double* db = d + fl.band[g];  // [t | ln_flux | ln_err | weight]
            const BandCols k = band_cols(bd.n);
            begin_pass();
            rc = band_request_dev(c, d_params, nb, db, bd.n, bd.nu_min, bd.nu_max, bd.num_points, c->d_series_flux.as<double>(), nullptr);
            if (rc == VAG_OK)
                rc = back(c->d_series_flux.as<double>(), bd.n, db + k.ln_flux, db + k.ln_err, db + k.weight, nullptr,
                          req.lim ? req.llay.band[g] : -1, req.noise ? req.nlay.band[g] : -1, req.noise ? req.nlay.band_present[g] : 0u,
                          req.tmpl ? req.tlay.band[g] : -1, req.tmpl ? req.tlay.band_present[g] : 0u, req.robust && req.rlay.band[g]);
        } break;
        case PassKind::Centroid: {  // centroid groups: one vag_sky_centroid_batch request each, after every flux pass
            const vag_centroid_obs& o = sky->groups[g];
            const double* ds = c->sky.d.as<double>() + req.slay.off[g];  // [nu | t | east | north | err_east | err_north | weight]
            const SixCols k = six_cols(o.n);
            if (c->d_skycmom.ensure(sizeof(double) * (size_t)nb * o.n * 6)) return VAG_E_HIP;
            rc = sky_group_stages(ds, k.rows, o.n);
            if (rc == VAG_OK) rc = centroid_request(c, d_params, nb, o.n, 1, c->d_skycmom.as<double>());
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_sky_back_kernel, dim3(nb), dim3(64), 0, st, c->d_skycmom.as<double>(), o.n, ds + k.rows, d_theta,
                                   ndim, d_prior, sky->pa_fixed, sky->east0_fixed, sky->north0_fixed, fit_pass());
                rc = end_pass();
            }
        } break;
        case PassKind::Vis: {  // visibility groups: one pass each, the chi^2 formed by the chi2 kernel
            const vag_visibility_obs& o = req.vis->groups[g];
            const VisLayout& lay = c->vis_layout[g];
            const double* ds = c->vis.d.as<double>() + lay.obs_off;  // [nu | t | ...]
            rc = sky_group_stages(ds, vis_cols(o).t, o.n_epochs);
            if (rc == VAG_OK) {
                SkyVisFitArgs va{};
                va.theta = d_theta;
                va.prior = d_prior;
                va.order = d_order;
                va.ndim = ndim;
                va.pa_fixed = sky ? sky->pa_fixed : 0.0;
                va.east0_fixed = sky ? sky->east0_fixed : 0.0;
                va.north0_fixed = sky ? sky->north0_fixed : 0.0;
                rc = vis_chi2_request(c, d_params, nb, o, lay, va);
            }
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_vis_back_kernel, dim3(nb), dim3(64), 0, st, c->d_vispart.as<double>(), lay.epoch_blk[o.n_epochs],
                                   fit_pass());
                rc = end_pass();
            }
        } break;
        case PassKind::Pol: {  // polarization groups: one pass each, the Stokes sums of sky_request
            if (g == 0) {  // the walkers' own field: once per call, in the evaluation order of d_params, before the first such pass
                if (c->d_polspec.ensure(sizeof(double) * 5 * (size_t)nb)) return VAG_E_HIP;  // [nb][4] spec | int [nb] flags
                hipLaunchKernelGGL(vag_fit_pol_spec_kernel, dim3((nb + 127) / 128), dim3(128), 0, st, d_theta, nb, ndim, d_prior, d_params,
                                   req.pol->b_fixed[0], req.pol->b_fixed[1], req.pol->pi_max_fixed[0], req.pol->pi_max_fixed[1], d_order,
                                   c->d_polspec.as<double>(), reinterpret_cast<int*>(c->d_polspec.as<double>() + 4 * (size_t)nb));
                HIPCHK(hipGetLastError());
            }
            const vag_polarization_obs& o = req.pol->groups[g];
            const double* ds = c->pol.d.as<double>() + req.play.off[g];  // [nu | t | q | u | err_q | err_u | weight]
            const SixCols k = six_cols(o.n);
            if (c->d_polstokes.ensure(sizeof(double) * (size_t)nb * o.n * 3)) return VAG_E_HIP;
            rc = sky_group_stages(ds, k.rows, o.n);
            if (rc == VAG_OK)
                rc = pol_stokes_request(c, d_params, nb, o.n, o.n_az > 0 ? o.n_az : 256, c->d_polspec.as<double>(),
                                        c->d_polstokes.as<double>());
            if (rc == VAG_OK) {
                const int* lk = (req.lim && req.llay.pol[g] >= 0) ? reinterpret_cast<const int*>(c->lim.d.as<double>() + req.llay.pol[g]) : nullptr;
                const int* bad = reinterpret_cast<const int*>(c->d_polspec.as<double>() + 4 * (size_t)nb);
                hipLaunchKernelGGL(lk ? vag_fit_pol_back_kernel<true> : vag_fit_pol_back_kernel<false>, dim3(nb), dim3(64), 0, st,
                                   c->d_polstokes.as<double>(), o.n, o.kind, ds + k.rows, bad, d_theta, ndim, d_prior,
                                   sky ? sky->pa_fixed : 0.0, fit_pass(), lk);
                rc = end_pass();
            }
        } break;
        case PassKind::Counts: {  // counts groups: one band request on the sample times each, then the Poisson term
            const vag_counts_obs& o = req.counts->groups[g];
            const double* dc = c->counts.d.as<double>() + req.clay.off[g];  // [t_sample | N | B | a | w | idx]
            const CountsCols k = counts_cols(o);
            if (room_for_flux((size_t)o.n_samples)) return VAG_E_HIP;
            begin_pass();
            // the band request takes two things from the batch's total work -- the number of (theta, phi) pairs per workgroup, and
            // from 262144 pairs on, for bands of at most 4 nodes, the row-per-lane kernel -- so a band group's flux depends on the
            // batch in its last bits; here both are pinned (COUNTS_PPB pairs, the workgroup kernel), and a walker's counts term is
            // the same bits alone and in any batch whose lattices fit the staged row (512 nodes)
            {
                CallMode<int> pin(c->ppb_pin, COUNTS_PPB);
                rc = band_request_dev(c, d_params, nb, dc, o.n_samples, o.nu_min, o.nu_max, o.num_points, c->d_series_flux.as<double>(),
                                      nullptr);
            }
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_back_counts_kernel, dim3(nb), dim3(64), 0, st, c->d_series_flux.as<double>(), o.n_samples, o.n,
                                   o.m, reinterpret_cast<const int*>(dc + k.idx), dc + k.N, dc + k.B, dc + k.a, dc + k.w, req.clay.const2[g],
                                   fit_pass(), next_order());
                rc = end_pass();
            }
        } break;
        case PassKind::Index: {  // spectral-index groups: the n K points as one series request each, then the slope term
            const vag_index_obs& o = req.index->groups[g];
            const double* di = c->index.d.as<double>() + req.ilay.off[g];  // [t n K | nu n K | s | sigma | w | c]
            const IndexCols k = index_cols(o);
            const size_t np = k.nu;  // (n K points: the length of the t column)
            double nu_pts[FITROWS_MAX_POINTS];  // K <= 8 distinct frequencies: the shared-node path of a short series
            if (room_for_flux(np)) return VAG_E_HIP;
            rc = series_group_flux(di, di + k.nu, np, short_series_nu(o.nu, (size_t)o.k, np, FITROWS_MAX_POINTS, nu_pts));
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_back_index_kernel, dim3(nb), dim3(64), 0, st, c->d_series_flux.as<double>(), o.n, o.k,
                                   di + k.value, di + k.err, di + k.weight, di + k.coef, o.ext_slope, d_av, fit_pass(), next_order());
                rc = end_pass();
            }
        } break;
        case PassKind::Fold: {  // fold groups: the n_samples J points as one series request each, then the folded Poisson term
            const vag_fold_obs& o = req.fold->groups[g];
            const double* df = c->fold.d.as<double>() + req.flay.off[g];  // [t ns J | nu ns J | A | sigma | exposure / m | N | B | w | idx]
            const FoldCols k = fold_cols(o);
            const size_t np = k.nu;  // (n_samples J points: the length of the t column)
            double nu_pts[FITROWS_MAX_POINTS];  // J <= 8 distinct frequencies: the shared-node path of a short series
            if (room_for_flux(np)) return VAG_E_HIP;
            rc = series_group_flux(df, df + k.nu, np, short_series_nu(o.nu, (size_t)o.J, np, FITROWS_MAX_POINTS, nu_pts));
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_back_fold_kernel, dim3(nb), dim3(64), 0, st, c->d_series_flux.as<double>(), o.n_samples, o.J, o.C,
                                   o.n, o.m, reinterpret_cast<const int*>(df + k.idx), df + k.A, o.sigma ? df + k.sigma : nullptr, df + k.eom,
                                   df + k.N, df + k.B, df + k.w, req.flay.const2[g], d_theta, ndim, d_prior, req.fold->n_h_fixed, fit_pass(),
                                   next_order());
                rc = end_pass();
            }
        } break;
        case PassKind::Cov: {  // correlated groups: the n rows as one series request each, then the whitened term
            const vag_cov_obs& o = req.cov->groups[g];
            const double* dv = c->cov.d.as<double>() + req.vlay.off[g];  // [t | nu | ln_flux | ext | Wt]
            const CovCols k = cov_cols(o);
            // (n <= 256 points: the shared-node path of a short series when the rows hold <= 8 distinct frequencies)
            if (room_for_flux((size_t)o.n)) return VAG_E_HIP;
            rc = series_group_flux(dv, dv + k.nu, (size_t)o.n, o.nu);
            if (rc == VAG_OK) {
                hipLaunchKernelGGL(vag_fit_back_cov_kernel, dim3(nb), dim3(64), 0, st, c->d_series_flux.as<double>(), o.n, dv + k.ln_flux,
                                   o.ext ? dv + k.ext : nullptr, dv + k.Wt, o.weight, d_av, fit_pass(), next_order());
                rc = end_pass();
            }
        } break;
        }
    }
    c->plan.n_models_capacity = n_cap;
    c->plan.n_models_invalid = n_inv;
    c->fit_stats_pending = true;
    if (rc == VAG_OK && order_made) {  // the order computed from this call's grids serves the next call of this size
        c->order_cur ^= 1;
        c->order_nb = nb;
    }
    return rc;
}

// One attempt of a likelihood call.  For its whole length the SSC tables' failures invalidate the walker instead of raising
// (ic_soft_fail, put back whichever way the passes are left); a call that did not end well -- a failed allocation in the middle
// of the passes included -- leaves no evaluation order to the next one.
static int loglike_body(vag_ctx* c, const FitRequest& req, const double* d_theta, int nb, int ndim, double* d_out, bool try_spec) {
    CallMode<bool> soft_fail(c->ic_soft_fail, true);
    const int rc = loglike_passes(c, req, d_theta, nb, ndim, d_out, try_spec);
    if (rc != VAG_OK) c->order_nb = 0;
    return rc;
}

// The call behind the uploads: the passes, repeated once on the waiting path when a planned-ahead call fails.  What loglike_dev, a
// sharded call and every half-step of the device sampler run on a request whose blocks are resident.
static int loglike_call(vag_ctx* c, const FitRequest& req, const double* d_theta, int nb, int ndim, double* d_out) {
    int rc = loglike_body(c, req, d_theta, nb, ndim, d_out, !c->count_work);
    if (rc == VAG_RETRY) rc = loglike_body(c, req, d_theta, nb, ndim, d_out, false);
    return rc;
}

// A likelihood call on device pointers: the scans, the checks, the uploads of every spec block the request holds, and the call
// (repeated once on the waiting path when a planned-ahead call fails).  The scans come first, as they always did in the entry points
// that scan: what they refuse is refused without a look at the context.
static int loglike_dev(vag_ctx* c, FitRequest& req, const double* d_theta, int nb, int ndim, double* d_out) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    int rc = req.spec ? fit_request_prepare(req) : VAG_OK;
    if (rc) return rc;
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!req.spec || !d_theta || !d_out) return set_err(VAG_E_INVALID, "null spec or device pointer");
    if (nb <= 0) return set_err(VAG_E_INVALID, "batch must be non-empty");
    HIPCHK(hipSetDevice(c->device));
    req.ndim = ndim;
    rc = upload_blocks(c, req);
    if (rc) return rc;
    return loglike_call(c, req, d_theta, nb, ndim, d_out);
}

// The host-pointer form: the scans (before anything goes to the device), then theta goes up, loglike_dev runs, the values come back.
static int loglike_host(vag_ctx* c, FitRequest& req, const double* theta, int nb, int ndim, double* out) {
    ApiLock api_lock(c);
    if (req.spec) {
        const int rc = fit_request_prepare(req);
        if (rc) return rc;
    }
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!req.spec || !theta || !out || ndim <= 0) return set_err(VAG_E_INVALID, "null spec, sample or output array");
    if (nb <= 0) return set_err(VAG_E_INVALID, "batch must be non-empty");
    HIPCHK(hipSetDevice(c->device));
    if (c->d_theta_in.ensure(sizeof(double) * (size_t)nb * (ndim + 1))) return VAG_E_HIP;
    double* d_theta = c->d_theta_in.as<double>();
    double* d_out = d_theta + (size_t)nb * ndim;
    HIPCHK(hipMemcpyAsync(d_theta, theta, sizeof(double) * (size_t)nb * ndim, hipMemcpyHostToDevice, c->stream));
    const int rc = loglike_dev(c, req, d_theta, nb, ndim, d_out);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    (void)collect_times(c);
    return VAG_OK;
}

int vag_loglike_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_sky_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const double* d_theta, int nb, int ndim,
                              double* d_out) {
    FitRequest r = fit_request(spec, sky);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_vis_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_pol_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_lim_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const double* d_theta, int nb, int ndim,
                              double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_noise_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_counts_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                 const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                 const vag_counts_fit_spec* counts, const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_index_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const double* d_theta, int nb,
                                int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_fold_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                               const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                               const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                               const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_tmpl_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                               const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                               const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                               const vag_template_fit_spec* tmpl, const double* d_theta, int nb, int ndim, double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold, tmpl);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

int vag_loglike_cov_batch_dev(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                              const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                              const vag_template_fit_spec* tmpl, const vag_cov_fit_spec* cov, const double* d_theta, int nb, int ndim,
                              double* d_out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold, tmpl, cov);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

// the request form (with the outlier groups): a null request is refused like a null spec
int vag_loglike_robust_batch_dev(vag_ctx* c, const vag_loglike_request* q, const double* d_theta, int nb, int ndim, double* d_out) {
    if (!q) return set_err(VAG_E_INVALID, "null request");
    FitRequest r = fit_request(q->spec, q->sky, q->vis, q->pol, q->lim, q->noise, q->counts, q->index, q->fold, q->tmpl, q->cov, q->robust);
    return loglike_dev(c, r, d_theta, nb, ndim, d_out);
}

// ---- the device sampler: the stretch move, the move mix, parallel tempering, nested sampling (kernels: vag_sampler.h, vag_moves.h,
//      vag_tempering.h, vag_nested.h; what the specs refuse and the arithmetic of the launches: vag_sampler_plan.h; the moves: the public header) ----

extern "C++" {  // (templates: this section lies within the extern "C" of the entry points)

// A sampler kernel of one lane per item on the context's stream; the key of `seed` leads every such kernel's arguments.
template <class Kernel, class... Args>
static int sampler_launch(vag_ctx* c, Kernel kernel, long long items, uint64_t seed, Args... args) {
    const SeedWords key = seed_words(seed);
    hipLaunchKernelGGL(kernel, dim3(lane_groups(items)), dim3(STRETCH_LANES), 0, c->stream, key.lo, key.hi, args...);
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

// The prologue of the eleven building-block entries, in this order: lock, handoff, nulls (`given`: the context, the spec and every
// buffer are there), the spec's checks, half (`who` null: the entry takes none), the device; then the launch.
template <class Check, class Launch>
static int sampler_entry(vag_ctx* c, bool given, const char* what, Check check, const char* who, int half, Launch launch) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!given) return set_err(VAG_E_INVALID, "null context, %s spec or buffer", what);
    if (const int rc = check()) return rc;
    if (const int rc = who ? half_check(who, half) : VAG_OK) return rc;
    HIPCHK(hipSetDevice(c->device));
    return launch();
}

// the scratch of a phase of nb proposals: one set for the four samplers, grown by whichever runs
struct SamplerScratch {
    double* prop;   // the proposals [nb][ndim]
    double* fresh;  // their ln p; under tempering and nested sampling their ln L [nb]
    double* aux;    // the ln of their Hastings factor (the move mix), their ln prior (tempering, nested sampling) [nb]
};

// The steps step0 .. step0 + n_steps - 1 of a run entry whose arguments have passed their checks: the scans and the uploads once,
// then per step what begins it and, per phase (`phases` of them: the two halves of a move, the walk steps of a nested iteration),
// propose, ONE likelihood call of the nb proposals, what the move runs behind it, accept; then what ends the step.  Between the steps
// there is no copy to the host and no stream synchronisation.  begin_step, accept and end_step are told whether the step is stored
// and which row it fills.
template <class BeginStep, class Propose, class Behind, class Accept, class EndStep>
static int sampler_run(vag_ctx* c, const vag_loglike_request* q, int ndim, int nb, int phases, int thin, bool storing, uint64_t step0,
                       int n_steps, BeginStep begin_step, Propose propose, Behind behind, Accept accept, EndStep end_step) {
    if (n_steps == 0) return VAG_OK;
    FitRequest req = fit_request(q->spec, q->sky, q->vis, q->pol, q->lim, q->noise, q->counts, q->index, q->fold, q->tmpl, q->cov, q->robust);
    int rc = fit_request_prepare(req);  // the scans, once per call of many steps
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    req.ndim = ndim;
    rc = upload_blocks(c, req);  // and the uploads
    if (rc) return rc;
    if (c->d_sampler_prop.ensure(sizeof(double) * (size_t)nb * ndim)) return VAG_E_HIP;
    if (c->d_sampler_fresh.ensure(sizeof(double) * (size_t)nb)) return VAG_E_HIP;
    if (c->d_sampler_aux.ensure(sizeof(double) * (size_t)nb)) return VAG_E_HIP;
    const SamplerScratch s{c->d_sampler_prop.as<double>(), c->d_sampler_fresh.as<double>(), c->d_sampler_aux.as<double>()};
    size_t row = 0;  // stored rows so far
    for (int k = 0; k < n_steps; ++k) {
        const uint64_t step = step0 + (uint64_t)k;
        const bool stored = storing && step_is_stored(step, thin);
        if ((rc = begin_step(step, stored, row))) return rc;
        for (int which = 0; which < phases; ++which) {
            if ((rc = propose(step, which, s))) return rc;
            if ((rc = loglike_call(c, req, s.prop, nb, ndim, s.fresh))) return rc;
            if ((rc = behind(s))) return rc;
            if ((rc = accept(step, which, s, stored, row))) return rc;
        }
        if ((rc = end_step(step, stored, row))) return rc;
        if (stored) ++row;
    }
    return VAG_OK;
}
static const auto no_hook = [](auto&&...) -> int { return VAG_OK; };  // a move with nothing to run there

}  // extern "C++"

// -- the stretch move --

static int stretch_propose(vag_ctx* c, const vag_stretch_spec* sp, uint64_t step, int which, const double* d_pos, double* d_prop) {
    const int half = half_of(sp->n_walkers);
    return sampler_launch(c, vag_stretch_propose_kernel, half, sp->seed, sp->a, (unsigned long long)step, which, half, sp->ndim, d_pos, d_prop);
}

static int stretch_accept(vag_ctx* c, const vag_stretch_spec* sp, uint64_t step, int which, const double* d_prop, const double* d_lp_new,
                          double* d_pos, double* d_lp, int64_t* d_accepted, double* d_chain_row, double* d_logp_row) {
    const int half = half_of(sp->n_walkers);
    return sampler_launch(c, vag_stretch_accept_kernel, half, sp->seed, sp->a, (unsigned long long)step, which, half, sp->ndim, d_prop,
                          d_lp_new, d_pos, d_lp, reinterpret_cast<long long*>(d_accepted), d_chain_row, d_logp_row);
}

int vag_stretch_propose_dev(vag_ctx* c, const vag_stretch_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop) {
    return sampler_entry(c, c && sp && d_pos && d_prop, "stretch", [&] { return stretch_spec_check(sp); }, "stretch move", half,
                         [&] { return stretch_propose(c, sp, step, half, d_pos, d_prop); });
}

int vag_stretch_accept_dev(vag_ctx* c, const vag_stretch_spec* sp, uint64_t step, int half, const double* d_prop, const double* d_lp_new,
                           double* d_pos, double* d_lp, int64_t* d_accepted) {
    return sampler_entry(c, c && sp && d_prop && d_lp_new && d_pos && d_lp && d_accepted, "stretch", [&] { return stretch_spec_check(sp); },
                         "stretch move", half,
                         [&] { return stretch_accept(c, sp, step, half, d_prop, d_lp_new, d_pos, d_lp, d_accepted, nullptr, nullptr); });
}

// (its own kernels, not the move mix with weights (1, 0, 0): the two round the acceptance margin differently)
int vag_stretch_run_dev(vag_ctx* c, const vag_loglike_request* q, const vag_stretch_spec* sp, uint64_t step0, int n_steps, double* d_pos,
                        double* d_lp, int64_t* d_accepted, double* d_chain, double* d_logp) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !q || !q->spec || !sp || !d_pos || !d_lp || !d_accepted)
        return set_err(VAG_E_INVALID, "null context, request, fit spec, stretch spec or buffer");
    if (const int rc = run_chain_check("stretch move", "the chain and its ln p", (d_chain != nullptr) + (d_logp != nullptr), 2)) return rc;
    if (const int rc = stretch_spec_check(sp)) return rc;
    if (const int rc = run_steps_check("stretch move", sp->ndim, q->spec->ndim, n_steps)) return rc;
    const int nw = sp->n_walkers, ndim = sp->ndim;
    return sampler_run(
        c, q, ndim, half_of(nw), HALF_PHASES, sp->thin, d_chain != nullptr, step0, n_steps, no_hook,
        [&](uint64_t step, int which, const SamplerScratch& s) { return stretch_propose(c, sp, step, which, d_pos, s.prop); }, no_hook,
        [&](uint64_t step, int which, const SamplerScratch& s, bool stored, size_t row) {
            return stretch_accept(c, sp, step, which, s.prop, s.fresh, d_pos, d_lp, d_accepted,
                                  stored ? d_chain + ensemble_row_offset(row, nw, ndim) : nullptr,
                                  stored ? d_logp + ensemble_row_offset(row, nw, 1) : nullptr);
        },
        no_hook);
}

// -- the move mix: stretch, differential evolution, snooker; the kind of a step is chosen here, so no kernel branches on it --

static int move_propose(vag_ctx* c, const vag_move_spec* sp, uint64_t step, int which, const double* d_pos, double* d_prop,
                        double* d_factor) {
    const int half = half_of(sp->n_walkers);
    switch (move_kind(sp, step)) {
        case MOVE_STRETCH:
            return sampler_launch(c, vag_move_stretch_propose_kernel, half, sp->seed, sp->a, (unsigned long long)step, which, half, sp->ndim,
                                  d_pos, d_prop, d_factor);
        case MOVE_DE:
            return sampler_launch(c, vag_de_propose_kernel, half, sp->seed, sp->gamma0 > 0.0 ? sp->gamma0 : de_gamma0(sp->ndim), sp->sigma,
                                  (unsigned long long)step, which, half, sp->ndim, d_pos, d_prop, d_factor);
        default:
            return sampler_launch(c, vag_snooker_propose_kernel, half, sp->seed, sp->gamma_snooker, (unsigned long long)step, which, half,
                                  sp->ndim, d_pos, d_prop, d_factor);
    }
}

static int move_accept(vag_ctx* c, const vag_move_spec* sp, uint64_t step, int which, const double* d_prop, const double* d_factor,
                       const double* d_lp_new, double* d_pos, double* d_lp, int64_t* d_accepted, double* d_chain_row, double* d_logp_row) {
    const int half = half_of(sp->n_walkers);
    return sampler_launch(c, vag_move_accept_kernel, half, sp->seed, (unsigned long long)step, which, half, sp->ndim, d_prop, d_factor,
                          d_lp_new, d_pos, d_lp, reinterpret_cast<long long*>(d_accepted), d_chain_row, d_logp_row);
}

int vag_move_propose_dev(vag_ctx* c, const vag_move_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop,
                         double* d_factor) {
    return sampler_entry(c, c && sp && d_pos && d_prop && d_factor, "move", [&] { return move_spec_check(sp); }, "move mix", half,
                         [&] { return move_propose(c, sp, step, half, d_pos, d_prop, d_factor); });
}

int vag_move_accept_dev(vag_ctx* c, const vag_move_spec* sp, uint64_t step, int half, const double* d_prop, const double* d_factor,
                        const double* d_lp_new, double* d_pos, double* d_lp, int64_t* d_accepted) {
    return sampler_entry(c, c && sp && d_prop && d_factor && d_lp_new && d_pos && d_lp && d_accepted, "move",
                         [&] { return move_spec_check(sp); }, "move mix", half, [&] {
                             return move_accept(c, sp, step, half, d_prop, d_factor, d_lp_new, d_pos, d_lp, d_accepted, nullptr, nullptr);
                         });
}

int vag_move_run_dev(vag_ctx* c, const vag_loglike_request* q, const vag_move_spec* sp, uint64_t step0, int n_steps, double* d_pos,
                     double* d_lp, int64_t* d_accepted, double* d_chain, double* d_logp) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !q || !q->spec || !sp || !d_pos || !d_lp || !d_accepted)
        return set_err(VAG_E_INVALID, "null context, request, fit spec, move spec or buffer");
    if (const int rc = run_chain_check("move mix", "the chain and its ln p", (d_chain != nullptr) + (d_logp != nullptr), 2)) return rc;
    if (const int rc = move_spec_check(sp)) return rc;
    if (const int rc = run_steps_check("move mix", sp->ndim, q->spec->ndim, n_steps)) return rc;
    const int nw = sp->n_walkers, ndim = sp->ndim;
    return sampler_run(
        c, q, ndim, half_of(nw), HALF_PHASES, sp->thin, d_chain != nullptr, step0, n_steps, no_hook,
        [&](uint64_t step, int which, const SamplerScratch& s) { return move_propose(c, sp, step, which, d_pos, s.prop, s.aux); }, no_hook,
        [&](uint64_t step, int which, const SamplerScratch& s, bool stored, size_t row) {
            return move_accept(c, sp, step, which, s.prop, s.aux, s.fresh, d_pos, d_lp, d_accepted,
                               stored ? d_chain + ensemble_row_offset(row, nw, ndim) : nullptr,
                               stored ? d_logp + ensemble_row_offset(row, nw, 1) : nullptr);
        },
        no_hook);
}

// -- parallel tempering --

// ln L and ln prior of the last likelihood call's nb walkers apart, from what loglike_body leaves by evaluation slot
static int fit_split(vag_ctx* c, int nb, double* d_lnl, double* d_lnprior) {
    const double* d_chi2 = c->d_chi2.as<double>();  // [chi2 | A_V | ln prior]
    hipLaunchKernelGGL(vag_fit_split_kernel, dim3((nb + STRETCH_LANES - 1) / STRETCH_LANES), dim3(STRETCH_LANES), 0, c->stream, d_chi2,
                       c->d_valid.as<int>(), d_chi2 + 2 * (size_t)nb, nb, c->last_order, d_lnl, d_lnprior);
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

int vag_loglike_split_dev(vag_ctx* c, const vag_loglike_request* q, const double* d_theta, int nb, int ndim, double* d_lnl,
                          double* d_lnprior) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);  // (closes behind the split, after the one of the call inside)
    if (!c || !q || !q->spec || !d_theta || !d_lnl || !d_lnprior) return set_err(VAG_E_INVALID, "null context, request, fit spec or device pointer");
    FitRequest req = fit_request(q->spec, q->sky, q->vis, q->pol, q->lim, q->noise, q->counts, q->index, q->fold, q->tmpl, q->cov, q->robust);
    const int rc = loglike_dev(c, req, d_theta, nb, ndim, d_lnl);  // (ln L + ln prior by walker, which the split then replaces)
    if (rc) return rc;
    return fit_split(c, nb, d_lnl, d_lnprior);
}

static int tempered_propose(vag_ctx* c, const vag_tempered_spec* sp, uint64_t step, int which, const double* d_pos, double* d_prop) {
    const int half = half_of(sp->n_walkers);
    return sampler_launch(c, vag_tempered_propose_kernel, (long long)sp->n_temps * half, sp->seed, sp->a, (unsigned long long)step, which,
                          half, sp->ndim, sp->n_temps, d_pos, d_prop);
}

static int tempered_accept(vag_ctx* c, const vag_tempered_spec* sp, const TemperLadder& ladder, uint64_t step, int which,
                           const double* d_prop, const double* d_lnl_new, const double* d_lnprior_new, double* d_pos, double* d_lnl,
                           double* d_lnprior, int64_t* d_accepted) {
    const int half = half_of(sp->n_walkers);
    return sampler_launch(c, vag_tempered_accept_kernel, (long long)sp->n_temps * half, sp->seed, sp->a, (unsigned long long)step, which,
                          half, sp->ndim, sp->n_temps, ladder, d_prop, d_lnl_new, d_lnprior_new, d_pos, d_lnl, d_lnprior,
                          reinterpret_cast<long long*>(d_accepted));
}

static int tempered_swap(vag_ctx* c, const vag_tempered_spec* sp, const TemperLadder& ladder, uint64_t step, double* d_pos, double* d_lnl,
                         double* d_lnprior, int64_t* d_swapped) {
    const int n_pairs = swap_pairs(sp->n_temps, step);
    if (n_pairs <= 0) return VAG_OK;
    return sampler_launch(c, vag_tempered_swap_kernel, (long long)n_pairs * sp->n_walkers, sp->seed, (unsigned long long)step,
                          sp->n_walkers, sp->ndim, n_pairs, ladder, d_pos, d_lnl, d_lnprior, reinterpret_cast<long long*>(d_swapped));
}

int vag_tempered_propose_dev(vag_ctx* c, const vag_tempered_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop) {
    TemperLadder ladder;
    return sampler_entry(c, c && sp && d_pos && d_prop, "tempered", [&] { return tempered_spec_check(sp, ladder); }, "tempering", half,
                         [&] { return tempered_propose(c, sp, step, half, d_pos, d_prop); });
}

int vag_tempered_accept_dev(vag_ctx* c, const vag_tempered_spec* sp, uint64_t step, int half, const double* d_prop,
                            const double* d_lnl_new, const double* d_lnprior_new, double* d_pos, double* d_lnl, double* d_lnprior,
                            int64_t* d_accepted) {
    TemperLadder ladder;
    return sampler_entry(c, c && sp && d_prop && d_lnl_new && d_lnprior_new && d_pos && d_lnl && d_lnprior && d_accepted, "tempered",
                         [&] { return tempered_spec_check(sp, ladder); }, "tempering", half, [&] {
                             return tempered_accept(c, sp, ladder, step, half, d_prop, d_lnl_new, d_lnprior_new, d_pos, d_lnl, d_lnprior,
                                                    d_accepted);
                         });
}

int vag_tempered_swap_dev(vag_ctx* c, const vag_tempered_spec* sp, uint64_t step, double* d_pos, double* d_lnl, double* d_lnprior,
                          int64_t* d_swapped) {
    TemperLadder ladder;
    return sampler_entry(c, c && sp && d_pos && d_lnl && d_lnprior && d_swapped, "tempered", [&] { return tempered_spec_check(sp, ladder); },
                         nullptr, 0, [&] { return tempered_swap(c, sp, ladder, step, d_pos, d_lnl, d_lnprior, d_swapped); });
}

int vag_tempered_run_dev(vag_ctx* c, const vag_loglike_request* q, const vag_tempered_spec* sp, uint64_t step0, int n_steps,
                         double* d_pos, double* d_lnl, double* d_lnprior, int64_t* d_accepted, int64_t* d_swapped, double* d_chain,
                         double* d_lnl_chain, double* d_lnprior_chain) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !q || !q->spec || !sp || !d_pos || !d_lnl || !d_lnprior || !d_accepted || !d_swapped)
        return set_err(VAG_E_INVALID, "null context, request, fit spec, tempered spec or buffer");
    if (const int rc = run_chain_check("tempering", "the chain, its ln L and its ln prior",
                                       (d_chain != nullptr) + (d_lnl_chain != nullptr) + (d_lnprior_chain != nullptr), 3))
        return rc;
    TemperLadder ladder;
    if (const int rc = tempered_spec_check(sp, ladder)) return rc;
    if (const int rc = run_steps_check("tempering", sp->ndim, q->spec->ndim, n_steps)) return rc;
    const int T = sp->n_temps, nw = sp->n_walkers, ndim = sp->ndim, nb = T * half_of(nw);
    const size_t replicas = (size_t)T * nw;
    return sampler_run(
        c, q, ndim, nb, HALF_PHASES, sp->thin, d_chain != nullptr, step0, n_steps, no_hook,  // all temperatures' proposals of the half in ONE likelihood call
        [&](uint64_t step, int which, const SamplerScratch& s) { return tempered_propose(c, sp, step, which, d_pos, s.prop); },
        [&](const SamplerScratch& s) { return fit_split(c, nb, s.fresh, s.aux); },
        [&](uint64_t step, int which, const SamplerScratch& s, bool, size_t) {
            return tempered_accept(c, sp, ladder, step, which, s.prop, s.fresh, s.aux, d_pos, d_lnl, d_lnprior, d_accepted);
        },
        [&](uint64_t step, bool stored, size_t row) -> int {
            if (const int rc = tempered_swap(c, sp, ladder, step, d_pos, d_lnl, d_lnprior, d_swapped)) return rc;
            if (!stored) return VAG_OK;  // the state after the exchanges (device-to-device, stream-ordered)
            HIPCHK(hipMemcpyAsync(d_chain + ladder_row_offset(row, T, nw, ndim), d_pos, sizeof(double) * replicas * ndim, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_lnl_chain + ladder_row_offset(row, T, nw, 1), d_lnl, sizeof(double) * replicas, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_lnprior_chain + ladder_row_offset(row, T, nw, 1), d_lnprior, sizeof(double) * replicas, hipMemcpyDeviceToDevice, c->stream));
            return VAG_OK;
        });
}

// -- nested sampling: an iteration is rank, retire, then `walk` phases of propose, the likelihood call, its split, accept --

static double nested_gamma0(const vag_nested_spec* sp) { return sp->gamma0 > 0.0 ? sp->gamma0 : de_gamma0(sp->ndim); }

static int nested_rank(vag_ctx* c, const vag_nested_spec* sp, const double* d_lnl, int32_t* d_order, double* d_lstar) {
    hipLaunchKernelGGL(vag_nested_rank_kernel, dim3(lane_groups(sp->n_live)), dim3(STRETCH_LANES), 0, c->stream, sp->n_live, d_lnl, d_order,
                       d_lstar);  // (no draw: the one sampler kernel without the seed's key)
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

static int nested_retire(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, const int32_t* d_order, double* d_live, double* d_lnl,
                         double* d_lnprior, double* d_dead_theta, double* d_dead_lnl, double* d_dead_lnprior) {
    return sampler_launch(c, vag_nested_retire_kernel, half_of(sp->n_live), sp->seed, nested_tick(it, sp->walk, 0), sp->n_live, sp->ndim,
                          d_order, d_live, d_lnl, d_lnprior, d_dead_theta, d_dead_lnl, d_dead_lnprior);
}

static int nested_propose(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_live,
                          double* d_prop) {
    return sampler_launch(c, vag_nested_propose_kernel, half_of(sp->n_live), sp->seed, nested_gamma0(sp), sp->sigma,
                          nested_tick(it, sp->walk, m), sp->n_live, sp->ndim, d_order, d_live, d_prop);
}

static int nested_accept(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_lstar,
                         const double* d_prop, const double* d_lnl_new, const double* d_lnprior_new, double* d_live, double* d_lnl,
                         double* d_lnprior, int64_t* d_accepted) {
    return sampler_launch(c, vag_nested_accept_kernel, half_of(sp->n_live), sp->seed, nested_tick(it, sp->walk, m), sp->n_live, sp->ndim,
                          d_order, d_lstar, d_prop, d_lnl_new, d_lnprior_new, d_live, d_lnl, d_lnprior,
                          reinterpret_cast<long long*>(d_accepted));
}

int vag_nested_rank_dev(vag_ctx* c, const vag_nested_spec* sp, const double* d_lnl, int32_t* d_order, double* d_lstar) {
    return sampler_entry(c, c && sp && d_lnl && d_order && d_lstar, "nested", [&] { return nested_spec_check(sp); }, nullptr, 0,
                         [&] { return nested_rank(c, sp, d_lnl, d_order, d_lstar); });
}

int vag_nested_retire_dev(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, const int32_t* d_order, double* d_live, double* d_lnl,
                          double* d_lnprior, double* d_dead_theta, double* d_dead_lnl, double* d_dead_lnprior) {
    return sampler_entry(c, c && sp && d_order && d_live && d_lnl && d_lnprior && d_dead_theta && d_dead_lnl && d_dead_lnprior, "nested",
                         [&] { return nested_spec_check(sp); }, nullptr, 0, [&] {
                             return nested_retire(c, sp, it, d_order, d_live, d_lnl, d_lnprior, d_dead_theta, d_dead_lnl, d_dead_lnprior);
                         });
}

int vag_nested_propose_dev(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_live,
                           double* d_prop) {
    return sampler_entry(c, c && sp && d_order && d_live && d_prop, "nested",
                         [&] { const int rc = nested_spec_check(sp); return rc ? rc : nested_walk_step_check(sp, m); }, nullptr, 0,
                         [&] { return nested_propose(c, sp, it, m, d_order, d_live, d_prop); });
}

int vag_nested_accept_dev(vag_ctx* c, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_lstar,
                          const double* d_prop, const double* d_lnl_new, const double* d_lnprior_new, double* d_live, double* d_lnl,
                          double* d_lnprior, int64_t* d_accepted) {
    return sampler_entry(c, c && sp && d_order && d_lstar && d_prop && d_lnl_new && d_lnprior_new && d_live && d_lnl && d_lnprior && d_accepted,
                         "nested", [&] { const int rc = nested_spec_check(sp); return rc ? rc : nested_walk_step_check(sp, m); }, nullptr, 0,
                         [&] {
                             return nested_accept(c, sp, it, m, d_order, d_lstar, d_prop, d_lnl_new, d_lnprior_new, d_live, d_lnl, d_lnprior,
                                                  d_accepted);
                         });
}

int vag_nested_run_dev(vag_ctx* c, const vag_loglike_request* q, const vag_nested_spec* sp, uint64_t it0, int n_iters, double* d_live,
                       double* d_lnl, double* d_lnprior, int64_t* d_accepted, double* d_dead_theta, double* d_dead_lnl,
                       double* d_dead_lnprior) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !q || !q->spec || !sp || !d_live || !d_lnl || !d_lnprior || !d_accepted || !d_dead_theta || !d_dead_lnl || !d_dead_lnprior)
        return set_err(VAG_E_INVALID, "null context, request, fit spec, nested spec or buffer");
    if (const int rc = nested_spec_check(sp)) return rc;
    if (const int rc = run_steps_check("nested sampling", sp->ndim, q->spec->ndim, n_iters)) return rc;
    if (n_iters == 0) return VAG_OK;
    const int n = sp->n_live, ndim = sp->ndim, nb = half_of(n);
    HIPCHK(hipSetDevice(c->device));
    if (c->d_nested_rank.ensure(sizeof(double) + sizeof(int32_t) * (size_t)n)) return VAG_E_HIP;
    double* d_lstar = c->d_nested_rank.as<double>();
    int32_t* d_order = reinterpret_cast<int32_t*>(d_lstar + 1);
    return sampler_run(
        c, q, ndim, nb, nested_phases(sp), 1, true, it0, n_iters,  // every iteration is stored: row = it - it0
        [&](uint64_t it, bool, size_t row) -> int {
            if (const int rc = nested_rank(c, sp, d_lnl, d_order, d_lstar)) return rc;
            return nested_retire(c, sp, it, d_order, d_live, d_lnl, d_lnprior, d_dead_theta + dead_row_offset(row, n, ndim),
                                 d_dead_lnl + dead_row_offset(row, n, 1), d_dead_lnprior + dead_row_offset(row, n, 1));
        },
        [&](uint64_t it, int phase, const SamplerScratch& s) { return nested_propose(c, sp, it, phase + 1, d_order, d_live, s.prop); },
        [&](const SamplerScratch& s) { return fit_split(c, nb, s.fresh, s.aux); },  // the K proposals, in rank order, in ONE likelihood call
        [&](uint64_t it, int phase, const SamplerScratch& s, bool, size_t row) {
            return nested_accept(c, sp, it, phase + 1, d_order, d_lstar, s.prop, s.fresh, s.aux, d_live, d_lnl, d_lnprior,
                                 d_accepted + dead_row_offset(row, n, 1));
        },
        no_hook);
}

// ---- chain autocorrelation (kernels and the definition's pieces: vag_chain_stats.h; the definition: the public header) ----

int vag_chain_autocorr_dev(vag_ctx* c, const vag_chain_spec* sp, const double* d_chain, double* d_rho, double* d_tau, int32_t* d_window) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !sp || !d_chain || !d_tau || !d_window) return set_err(VAG_E_INVALID, "null context, chain spec or buffer");
    if (sp->n_rows < 2) return set_err(VAG_E_INVALID, "chain autocorrelation: n_rows must be >= 2, got %lld", (long long)sp->n_rows);
    if (sp->nwalkers < 1 || sp->ndim < 1)
        return set_err(VAG_E_INVALID, "chain autocorrelation: nwalkers and ndim must be >= 1, got %d and %d", sp->nwalkers, sp->ndim);
    const long long series = (long long)sp->nwalkers * sp->ndim;
    if (sp->row_stride < series)
        return set_err(VAG_E_INVALID, "chain autocorrelation: row_stride must be >= nwalkers * ndim = %lld, got %lld", series, (long long)sp->row_stride);
    if (sp->max_lag < 1 || (long long)sp->max_lag > (long long)sp->n_rows - 1)
        return set_err(VAG_E_INVALID, "chain autocorrelation: max_lag must be 1..n_rows - 1 = %lld, got %d", (long long)sp->n_rows - 1, sp->max_lag);
    if (!std::isfinite(sp->c) || !(sp->c > 0.0)) return set_err(VAG_E_INVALID, "chain autocorrelation: c must be finite and > 0, got %g", sp->c);
    const long long lags = (long long)sp->max_lag + 1;
    if (series > VAG_CHAIN_SCRATCH_MAX / 8 / lags)
        return set_err(VAG_E_CAPACITY, "chain autocorrelation: the lag sums (max_lag + 1) * nwalkers * ndim * 8 = %lld * %lld * 8 bytes exceed %lld", lags,
                       series, (long long)VAG_CHAIN_SCRATCH_MAX);
    HIPCHK(hipSetDevice(c->device));
    const int S = (int)series, L = sp->max_lag, D = sp->ndim;  // (S < 2^27 under the cap)
    if (c->d_chain_stats.ensure(sizeof(double) * ((size_t)S + (size_t)lags * S + (size_t)lags * D))) return VAG_E_HIP;
    double* d_mean = c->d_chain_stats.as<double>();
    double* d_lag = d_mean + S;
    double* d_pooled = d_lag + (size_t)lags * S;
    const unsigned groups = (unsigned)((S + CHAIN_LANES - 1) / CHAIN_LANES);
    const unsigned tiles = (unsigned)((lags + VAG_CHAIN_TILE - 1) / VAG_CHAIN_TILE);
    hipLaunchKernelGGL(vag_chain_mean_kernel, dim3(groups), dim3(CHAIN_LANES), 0, c->stream, d_chain, (long long)sp->n_rows,
                       (long long)sp->row_stride, S, d_mean);
    HIPCHK(hipGetLastError());
    const unsigned tile_groups = (tiles + VAG_CHAIN_WAVES - 1) / VAG_CHAIN_WAVES;  // (groups * tile_groups < 2^23 under the cap)
    hipLaunchKernelGGL(vag_chain_acf_kernel, dim3(groups * tile_groups), dim3(CHAIN_LANES, VAG_CHAIN_WAVES), 0, c->stream, d_chain,
                       (long long)sp->n_rows, (long long)sp->row_stride, S, (int)groups, L, d_mean, d_lag);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(vag_chain_pool_kernel, dim3((unsigned)((lags * D + 255) / 256)), dim3(256), 0, c->stream, d_lag, sp->nwalkers, D, L,
                       d_pooled);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(vag_chain_tau_kernel, dim3((unsigned)((D + CHAIN_LANES - 1) / CHAIN_LANES)), dim3(CHAIN_LANES), 0, c->stream, d_pooled, D,
                       L, sp->c, d_rho ? d_rho : d_pooled, d_tau, reinterpret_cast<int*>(d_window));
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

// ---- posterior-predictive bands (kernels and the definition's pieces: vag_predict.h; the definition: the public header) ----

static int quantile_spec_check(const vag_quantile_spec* qs) {
    if (qs->nq < 1 || qs->nq > VAG_PREDICT_MAX_Q)
        return set_err(VAG_E_INVALID, "column quantiles: nq must be 1..%d, got %d", VAG_PREDICT_MAX_Q, qs->nq);
    for (int k = 0; k < qs->nq; ++k)
        if (!(qs->q[k] >= 0.0 && qs->q[k] <= 1.0))
            return set_err(VAG_E_INVALID, "column quantiles: q[%d] must be in [0, 1], got %g", k, qs->q[k]);
    return VAG_OK;
}

static int quantile_shape_check(int S, long long M) {
    if (S < 1 || M < 1) return set_err(VAG_E_INVALID, "column quantiles: draws and columns must be >= 1, got %d and %lld", S, M);
    if (S > VAG_PREDICT_MAX_DRAWS)
        return set_err(VAG_E_CAPACITY, "column quantiles: %d draws exceed VAG_PREDICT_MAX_DRAWS = %d", S, VAG_PREDICT_MAX_DRAWS);
    if (M > VAG_PREDICT_MAX_VALUES / S)
        return set_err(VAG_E_CAPACITY, "column quantiles: draws * columns = %d * %lld values exceed VAG_PREDICT_MAX_VALUES = %lld", S, M,
                       (long long)VAG_PREDICT_MAX_VALUES);
    return VAG_OK;
}

// The two launches of the quantile stage on checked arguments; d_flags: int32 [S] of context scratch for the draws' validity.
static int column_quantiles(vag_ctx* c, const vag_quantile_spec* qs, const double* d_F, int S, int M, const int* d_valid_in, int* d_flags,
                            double* d_out, int* d_valid_out, int* d_n_valid) {
    PredictQ q{};
    q.nq = qs->nq;
    for (int k = 0; k < qs->nq; ++k) q.q[k] = qs->q[k];
    hipLaunchKernelGGL(vag_predict_valid_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, c->stream, d_F, S, M, d_valid_in, d_flags,
                       d_valid_out);
    HIPCHK(hipGetLastError());
    const int P = predict_network_size(S), T = predict_tile_columns(S);
    const int lanes = std::min(1024, std::max(64, P * T / 2));
    const size_t lds = 16 + sizeof(double) * (size_t)P * T;  // (<= 16 + VAG_PREDICT_LDS_BYTES)
    hipLaunchKernelGGL(vag_predict_quantile_kernel, dim3((unsigned)((M + T - 1) / T)), dim3(lanes), lds, c->stream, d_F, S, M, d_flags, P,
                       T, q, d_out, d_n_valid);
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

int vag_column_quantiles_dev(vag_ctx* c, const vag_quantile_spec* qs, const double* d_F, int S, int M, const int32_t* d_valid_in,
                             double* d_out, int32_t* d_valid_out, int32_t* d_n_valid) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !qs || !d_F || !d_out || !d_n_valid) return set_err(VAG_E_INVALID, "null context, quantile spec or buffer");
    if (const int rc = quantile_spec_check(qs)) return rc;
    if (const int rc = quantile_shape_check(S, M)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (c->d_predict.ensure(sizeof(int) * (size_t)S)) return VAG_E_HIP;
    c->handoff_dirty = true;
    return column_quantiles(c, qs, d_F, S, M, reinterpret_cast<const int*>(d_valid_in), c->d_predict.as<int>(), d_out,
                            reinterpret_cast<int*>(d_valid_out), reinterpret_cast<int*>(d_n_valid));
}

int vag_predict_bands_dev(vag_ctx* c, const vag_fit_spec* spec, const double* d_theta, int S, int ndim, const double* d_t, int nt,
                          const double* d_nu, int nnu, const double* d_ext, const vag_quantile_spec* qs, double* d_bands, double* d_draws,
                          int32_t* d_valid, int32_t* d_n_valid) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !spec || !d_theta || !d_t || !d_nu || !qs || !d_bands || !d_n_valid)
        return set_err(VAG_E_INVALID, "null context, fit spec, quantile spec or buffer");
    if (ndim != spec->ndim || ndim < 1 || ndim > 16) return set_err(VAG_E_INVALID, "predictive bands: ndim must match spec and be in 1..16");
    for (int d = 0; d < ndim; ++d) {
        const int s = spec->slot[d];
        if (s < 0 || (s >= VAG_P_COUNT && s < VAG_P_RVS_EPS_E) || (s > VAG_P_MAG_Q && s < VAG_P_A_V))
            return set_err(VAG_E_INVALID, "predictive bands: bad parameter slot %d of parameter %d", s, d);
    }
    if (nt < 1 || nnu < 1) return set_err(VAG_E_INVALID, "predictive bands: empty time or frequency array");
    if (const int rc = quantile_spec_check(qs)) return rc;
    const long long M = (long long)nnu * nt;
    if (const int rc = quantile_shape_check(S, M)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t n_flux = d_draws ? 0 : (size_t)S * (size_t)M;
    if (c->d_params.ensure(sizeof(vag_model_params) * (size_t)S)) return VAG_E_HIP;
    if (c->d_predict.ensure(sizeof(double) * ((size_t)S + n_flux) + sizeof(int) * 2 * (size_t)S)) return VAG_E_HIP;
    double* d_av = c->d_predict.as<double>();
    double* draws = d_draws ? d_draws : d_av + S;
    int* d_ok = reinterpret_cast<int*>(d_av + S + n_flux);
    int* d_flags = d_ok + S;
    vag_model_params* d_params = c->d_params.as<vag_model_params>();
    PredictSlots sl{};
    for (int d = 0; d < ndim; ++d) sl.slot[d] = spec->slot[d], sl.is_log[d] = spec->is_log[d];
    c->handoff_dirty = true;
    hipLaunchKernelGGL(vag_predict_front_kernel, dim3((unsigned)((S + 127) / 128)), dim3(128), 0, c->stream, spec->base, d_theta, S, ndim, sl,
                       spec->a_v_fixed, d_params, d_av);
    HIPCHK(hipGetLastError());
    c->mixed_flags_seen = false;  // (the draws share the base's flags: one flag set)
    if (const int rc = grid_dev_body(c, d_params, S, d_t, nt, d_nu, nnu, draws)) return rc;
    hipLaunchKernelGGL(vag_predict_back_kernel, dim3((unsigned)S), dim3(256), 0, c->stream, draws, nnu, nt, d_ext, d_av,
                       c->d_meta.as<VagGridMeta>(), c->d_row_status.as<int>(), c->d_row_off.as<int>(), d_ok);
    HIPCHK(hipGetLastError());
    return column_quantiles(c, qs, draws, S, (int)M, d_ok, d_flags, d_bands, reinterpret_cast<int*>(d_valid),
                            reinterpret_cast<int*>(d_n_valid));
}

__global__ void vag_model_cost_kernel(const VagGridMeta* __restrict__ meta, int nb, double* __restrict__ cost,
                                      const int* __restrict__ order /* evaluation slot -> walker of the last batch, or null */) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nb) return;
    const VagGridMeta M = meta[m];
    cost[order ? order[m] : m] = M.status == 0 ? (double)M.n_theta * (double)M.n_phi_eff * (double)M.n_t : 0.0;
}

int vag_last_model_costs_dev(vag_ctx* c, int nb, double* d_cost) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c || !d_cost) return set_err(VAG_E_INVALID, "null context or buffer");
    if (nb <= 0 || nb != c->nb || !c->d_meta.p) return set_err(VAG_E_INVALID, "no batch of %d models has been evaluated on this context", nb);
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(vag_model_cost_kernel, dim3((nb + 127) / 128), dim3(128), 0, c->stream, c->d_meta.as<VagGridMeta>(), nb, d_cost,
                       c->order_active ? c->last_order : nullptr);
    HIPCHK(hipGetLastError());
    return VAG_OK;
}

// ---- sharded log_prob_batch: the deal, this rank's block, the scatter after the caller's all-gather (ABI v9) ----

// One wavefront per position-or-walker m.  m < nb_all: walker m's rank q by counting (stable, descending cost; without costs
// every walker counts 1 and q = m), its (rank r, slot s) of the boustrophedon deal, table[r * per + s] = m, and -- when r is this
// process's rank -- its theta row into the rank's compact block.  m >= nb_all: padding positions of the last sweep, table = -1.
__global__ void __launch_bounds__(256)
vag_shard_deal_kernel(const double* __restrict__ cost /* [nb_all] or null */, const double* __restrict__ theta_all, int nb_all,
                      int ndim, int rank, int world, int per, int* __restrict__ table, double* __restrict__ theta_mine) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= world * per) return;
    int q = m;
    if (m < nb_all && cost) {
        const double mine = cost[m];
        q = 0;
        for (int i0 = 0; i0 < nb_all; i0 += 64) {
            const int i = i0 + lane;
            const double c = i < nb_all ? cost[i] : -1.0;
            q += __popcll(__ballot(c > mine || (c == mine && i < m)));
        }
    }
    const int s = q / world, k = q - s * world;
    const int r = (s & 1) ? world - 1 - k : k;
    if (lane == 0) table[r * per + s] = m < nb_all ? m : -1;
    if (m < nb_all && r == rank && lane < ndim) theta_mine[(size_t)s * ndim + lane] = theta_all[(size_t)m * ndim + lane];
}

// block[s] = {ln L, cost} of this rank's slot s (cost = the (theta, phi, t) cell count of vag_last_model_costs_dev), {NaN, 0} for padding
__global__ void vag_shard_pack_kernel(const double* __restrict__ ll, const VagGridMeta* __restrict__ meta,
                                      const int* __restrict__ order /* evaluation slot -> block slot, or null */, int n_mine, int per,
                                      double* __restrict__ block) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= per) return;
    if (s < n_mine) {
        const VagGridMeta M = meta[s];
        block[2 * (size_t)s] = ll[s];
        block[2 * (size_t)(order ? order[s] : s) + 1] = M.status == 0 ? (double)M.n_theta * (double)M.n_phi_eff * (double)M.n_t : 0.0;
    } else {
        block[2 * (size_t)s] = NAN;
        block[2 * (size_t)s + 1] = 0.0;
    }
}

// One workgroup: ln L back into walker order, the gathered costs kept for the next deal (a walker that was not evaluated is
// assumed average: the mean of the positive costs, or 1).
__global__ void __launch_bounds__(1024)
vag_shard_finish_kernel(const double* __restrict__ gathered, const int* __restrict__ table, int n_slots, double* __restrict__ out,
                        double* __restrict__ cost) {
    __shared__ double s_sum[16];
    __shared__ double s_cnt[16];
    double sum = 0, cnt = 0;
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
        const int w = table[i];
        if (w < 0) continue;
        out[w] = gathered[2 * (size_t)i];
        const double cw = gathered[2 * (size_t)i + 1];
        if (cw > 0) sum += cw, cnt += 1;
    }
    sum = vag::wave_sum(sum);
    cnt = vag::wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum, s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    sum = 0, cnt = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) sum += s_sum[i], cnt += s_cnt[i];
    const double mean = cnt > 0 ? sum / cnt : 1.0;
    for (int i = threadIdx.x; i < n_slots; i += blockDim.x) {
        const int w = table[i];
        if (w < 0) continue;
        const double cw = gathered[2 * (size_t)i + 1];
        cost[w] = cw > 0 ? cw : mean;
    }
}

static int shard_begin(vag_ctx* c, const vag_fit_spec* spec, const double* d_theta_all, int nb_all, int ndim, int rank, int world,
                       double* d_block, uint64_t* ticket) {
    if (!c || !spec || !d_theta_all || !d_block) return set_err(VAG_E_INVALID, "null context, spec or buffer");
    if (nb_all <= 0) return set_err(VAG_E_INVALID, "batch must be non-empty");
    if (world <= 0 || rank < 0 || rank >= world) return set_err(VAG_E_INVALID, "rank %d outside a world of %d", rank, world);
    if (ndim <= 0 || ndim > 16) return set_err(VAG_E_INVALID, "ndim must be 1..16");
    HIPCHK(hipSetDevice(c->device));
    const int per = (nb_all + world - 1) / world;
    // slots of this rank that hold a walker: positions q = s * world + k(s) < nb_all
    int n_mine = 0;
    for (int s = 0; s < per; ++s) {
        const int k = (s & 1) ? world - 1 - rank : rank;
        if ((long long)s * world + k < nb_all) ++n_mine;
    }
    if (c->d_shard_theta.ensure(sizeof(double) * (size_t)per * ndim)) return VAG_E_HIP;
    if (c->d_shard_ll.ensure(sizeof(double) * (size_t)per)) return VAG_E_HIP;
    // every rank needs the same deal, whether or not it holds a walker: the key of the costs is the spec's content hash
    FitRequest req = fit_request(spec);  // (the fit block alone, no optional block)
    req.ndim = ndim;
    if (const int rc = upload_blocks(c, req, true)) return rc;
    int entry = -1, victim = -1;
    for (int i = 0; i < 4; ++i) {
        const vag_ctx::ShardCosts& e = c->shard_costs[i];
        if (e.nb == nb_all && e.world == world && e.hash == c->fit.hash) entry = i;
        if (e.in_flight == 0 && (victim < 0 || e.used < c->shard_costs[victim].used)) victim = i;
    }
    int slot = -1;  // a free flight slot, the least recently dealt one
    for (int i = 0; i < 8; ++i)
        if (!c->shard_flights[i].in_use && (slot < 0 || c->shard_flights[i].ticket < c->shard_flights[slot].ticket)) slot = i;
    // the unticketed form deals a key anew when it is dealt again before its finish (the earlier block never goes through a finish)
    bool replaces = false;
    for (int i = 0; i < 8 && !ticket && entry >= 0; ++i)
        if (c->shard_flights[i].in_use && c->shard_flights[i].unticketed && c->shard_flights[i].key == entry) slot = i, replaces = true;
    if (slot < 0) return set_err(VAG_E_INVALID, "eight sharded calls wait for their finish on this context");
    if (entry < 0) {
        if (victim < 0) return set_err(VAG_E_INVALID, "sharded calls of four other fits wait for their finish on this context");
        entry = victim;
        c->shard_costs[entry].nb = nb_all;
        c->shard_costs[entry].world = world;
        c->shard_costs[entry].hash = c->fit.hash;
        c->shard_costs[entry].valid = false;  // until its first call finishes
        if (c->shard_last == entry) c->shard_last = -1;
    }
    // ranking by counting is O(nb_all^2 / 64) per call: beyond 16384 walkers the deal stays by position (equal counts)
    const bool ranked = c->shard_costs[entry].valid && nb_all <= 16384;
    c->shard_costs[entry].used = ++c->shard_clock;
    vag_ctx::ShardFlight& fl = c->shard_flights[slot];
    if (c->shard_costs[entry].cost.ensure(sizeof(double) * (size_t)nb_all)) return VAG_E_HIP;
    if (fl.table.ensure(sizeof(int) * (size_t)world * per)) return VAG_E_HIP;
    hipLaunchKernelGGL(vag_shard_deal_kernel, dim3((world * per + 3) / 4), dim3(256), 0, c->stream,
                       ranked ? c->shard_costs[entry].cost.as<double>() : nullptr, d_theta_all, nb_all, ndim, rank, world, per,
                       fl.table.as<int>(), c->d_shard_theta.as<double>());
    HIPCHK(hipGetLastError());
    fl.ticket = c->shard_clock;
    fl.key = entry;
    fl.nb = nb_all;
    fl.world = world;
    c->shard_last_dealt = slot;  // (kept for inspection even if the evaluation below fails)
    const int* d_order = nullptr;
    if (n_mine > 0) {
        const int rc = loglike_call(c, req, c->d_shard_theta.as<double>(), n_mine, ndim, c->d_shard_ll.as<double>());
        if (rc) {  // (no block went out: there is nothing to finish, the slot is free)
            if (replaces) fl.in_use = false, --c->shard_costs[entry].in_flight;
            return rc;
        }
        d_order = c->order_active ? c->last_order : nullptr;
    }
    hipLaunchKernelGGL(vag_shard_pack_kernel, dim3((per + 127) / 128), dim3(128), 0, c->stream, c->d_shard_ll.as<double>(),
                       c->d_meta.as<VagGridMeta>(), d_order, n_mine, per, d_block);
    HIPCHK(hipGetLastError());
    fl.in_use = true;
    fl.unticketed = !ticket;
    if (!replaces) ++c->shard_costs[entry].in_flight;
    if (ticket) *ticket = fl.ticket;
    return VAG_OK;
}

// ticket 0: the oldest call in flight of this shape (the v9 form; right when calls of equal shape finish in the order of their deals)
static int shard_end(vag_ctx* c, uint64_t ticket, const double* d_gathered, int nb_all, int world, double* d_out) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    const bool abandon = ticket && !d_gathered && !d_out;  // the caller's collective failed: release the call, keep the costs as they are
    if (!abandon && (!d_gathered || !d_out)) return set_err(VAG_E_INVALID, "null context or buffer");
    int slot = -1;
    for (int i = 0; i < 8 && nb_all > 0; ++i) {
        const vag_ctx::ShardFlight& f = c->shard_flights[i];
        if (!f.in_use) continue;
        if (ticket ? f.ticket == ticket : (f.nb == nb_all && f.world == world && (slot < 0 || f.ticket < c->shard_flights[slot].ticket))) slot = i;
    }
    if (slot < 0) {
        if (ticket) return set_err(VAG_E_INVALID, "no sharded call with ticket %llu is waiting for its finish", (unsigned long long)ticket);
        return set_err(VAG_E_INVALID, "no vag_loglike_shard_dev call of %d walkers over %d ranks is waiting for its finish", nb_all, world);
    }
    vag_ctx::ShardFlight& fl = c->shard_flights[slot];
    if (fl.nb != nb_all || fl.world != world)
        return set_err(VAG_E_INVALID, "ticket %llu was dealt for %d walkers over %d ranks, not %d over %d", (unsigned long long)ticket, fl.nb, fl.world,
                       nb_all, world);
    vag_ctx::ShardCosts& key = c->shard_costs[fl.key];
    if (abandon) {
        --key.in_flight;
        fl.in_use = false;
        return VAG_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    const int per = (nb_all + world - 1) / world;
    hipLaunchKernelGGL(vag_shard_finish_kernel, dim3(1), dim3(1024), 0, c->stream, d_gathered, fl.table.as<int>(), world * per, d_out,
                       key.cost.as<double>());
    HIPCHK(hipGetLastError());
    key.valid = true;
    --key.in_flight;
    fl.in_use = false;
    c->shard_last = fl.key;
    return VAG_OK;
}

int vag_loglike_shard_dev(vag_ctx* c, const vag_fit_spec* spec, const double* d_theta_all, int nb_all, int ndim, int rank, int world,
                          double* d_block) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    return shard_begin(c, spec, d_theta_all, nb_all, ndim, rank, world, d_block, nullptr);
}

int vag_loglike_shard_finish_dev(vag_ctx* c, const double* d_gathered, int nb_all, int world, double* d_out) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    return shard_end(c, 0, d_gathered, nb_all, world, d_out);
}

int vag_loglike_shard_begin_dev(vag_ctx* c, const vag_fit_spec* spec, const double* d_theta_all, int nb_all, int ndim, int rank, int world,
                                double* d_block, uint64_t* ticket) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!ticket) return set_err(VAG_E_INVALID, "null ticket");
    *ticket = 0;
    return shard_begin(c, spec, d_theta_all, nb_all, ndim, rank, world, d_block, ticket);
}

int vag_loglike_shard_end_dev(vag_ctx* c, uint64_t ticket, const double* d_gathered, int nb_all, int world, double* d_out) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!ticket) return set_err(VAG_E_INVALID, "ticket 0 names no call");
    return shard_end(c, ticket, d_gathered, nb_all, world, d_out);
}

int vag_loglike_shard_state_dev(vag_ctx* c, int nb_all, int world, int32_t* d_table, double* d_cost) {
    ApiLock api_lock(c);
    HandoffScope handoff(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    const int per = world > 0 ? (nb_all + world - 1) / world : 0;
    const int ld = c->shard_last_dealt;
    if (nb_all <= 0 || world <= 0 || ld < 0 || c->shard_flights[ld].nb != nb_all || c->shard_flights[ld].world != world ||
        c->shard_flights[ld].table.cap < sizeof(int) * (size_t)world * per)
        return set_err(VAG_E_INVALID, "no deal of %d walkers over %d ranks on this context", nb_all, world);
    HIPCHK(hipSetDevice(c->device));
    if (d_table)
        HIPCHK(hipMemcpyAsync(d_table, c->shard_flights[ld].table.p, sizeof(int) * (size_t)world * per, hipMemcpyDeviceToDevice, c->stream));
    if (d_cost) {
        if (c->shard_last < 0 || !c->shard_costs[c->shard_last].valid || c->shard_costs[c->shard_last].nb != nb_all || c->shard_costs[c->shard_last].world != world)
            return set_err(VAG_E_INVALID, "no finished sharded call of %d walkers over %d ranks on this context", nb_all, world);
        HIPCHK(hipMemcpyAsync(d_cost, c->shard_costs[c->shard_last].cost.p, sizeof(double) * (size_t)nb_all, hipMemcpyDeviceToDevice, c->stream));
    }
    return VAG_OK;
}

int vag_loglike_batch(vag_ctx* c, const vag_fit_spec* spec, const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_sky_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const double* theta, int nb, int ndim,
                          double* out) {
    FitRequest r = fit_request(spec, sky);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_vis_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_pol_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_lim_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_noise_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                            const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                            const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_counts_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                             const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                             const vag_counts_fit_spec* counts, const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_index_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                            const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                            const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const double* theta, int nb, int ndim,
                            double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_fold_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                           const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                           const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                           const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_tmpl_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                           const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                           const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                           const vag_template_fit_spec* tmpl, const double* theta, int nb, int ndim, double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold, tmpl);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_cov_batch(vag_ctx* c, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                          const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                          const vag_template_fit_spec* tmpl, const vag_cov_fit_spec* cov, const double* theta, int nb, int ndim,
                          double* out) {
    FitRequest r = fit_request(spec, sky, vis, pol, lim, noise, counts, index, fold, tmpl, cov);
    return loglike_host(c, r, theta, nb, ndim, out);
}

int vag_loglike_robust_batch(vag_ctx* c, const vag_loglike_request* q, const double* theta, int nb, int ndim, double* out) {
    if (!q) return set_err(VAG_E_INVALID, "null request");
    FitRequest r = fit_request(q->spec, q->sky, q->vis, q->pol, q->lim, q->noise, q->counts, q->index, q->fold, q->tmpl, q->cov, q->robust);
    return loglike_host(c, r, theta, nb, ndim, out);
}

// ------------------------------------------------------------------------------------------------
// Coalescer (ABI v11, opt-in): the reference's own calling pattern is a thread pool with one Model per thread and the GIL released
// inside the compute methods (pybind/pybind.cpp:424-448; VegasAfterglow/fitting/samplers.py:59-70 maps eval_one over a
// ThreadPoolExecutor).  Serialised on one GPU context that pattern runs at one light curve per call latency.  The *_coalesced entry
// points take ONE model each, block the calling thread, and gather the calls that are waiting at the same time -- same request
// (method, times, frequencies / band) -- into one batch call of the ordinary entry point; every caller gets its own model's slice.
// Group commit: the first caller to find no batch forming becomes the leader, waits up to co_wait_us for company (none needed while
// the GPU is busy: whoever arrives during a batch call is queued for the next one), runs the batch under the context lock, hands
// the results out and promotes the next leader.  A batch that fails as a whole (one member's grid over capacity, say) is repeated
// member by member, so a caller only ever sees the error of its own model.
// ------------------------------------------------------------------------------------------------
struct CoalesceRequest {
    int kind;  // 0 grid, 1 series, 2 band; +4: components form (out4) instead of the total (out)
    const vag_model_params* p;
    const double *t, *nu;
    int nt, nnu;  // series: nnu == nt
    double nu_min, nu_max;
    int num_nu;
    double* out;
    double* const* out4;
    int rc = VAG_OK;
    std::string err;
    bool done = false, promoted = false;
    std::condition_variable cv;  // this member's own wake-up (done / promoted): an arrival or a finished batch wakes who it concerns,
                                 // not every sleeping thread of the pool (r05: one shared condition variable with notify_all made
                                 // each arrival wake ~20 sleepers, each of which took the mutex to find nothing for it)
    bool same_request(const CoalesceRequest& o) const {
        if (kind != o.kind || nt != o.nt || nnu != o.nnu) return false;
        if ((kind & 3) == 2) return nu_min == o.nu_min && nu_max == o.nu_max && num_nu == o.num_nu && (t == o.t || !std::memcmp(t, o.t, sizeof(double) * nt));
        return (t == o.t || !std::memcmp(t, o.t, sizeof(double) * nt)) && (nu == o.nu || !std::memcmp(nu, o.nu, sizeof(double) * nnu));
    }
    size_t out_len() const { return (kind & 3) == 0 ? (size_t)nt * nnu : (size_t)nt; }
};

static int coalesce_run_one(vag_ctx* c, CoalesceRequest& r, const vag_model_params* params, int nb, double* out, double* const* out4) {
    switch (r.kind) {
        case 0: return vag_flux_density_grid_batch(c, params, nb, r.t, r.nt, r.nu, r.nnu, out);
        case 4: return vag_flux_density_grid_components4_batch(c, params, nb, r.t, r.nt, r.nu, r.nnu, out4);
        case 1: return vag_flux_density_batch(c, params, nb, r.t, r.nu, r.nt, out);
        case 5: return vag_flux_density_components4_batch(c, params, nb, r.t, r.nu, r.nt, out4);
        case 2: return vag_flux_batch(c, params, nb, r.t, r.nt, r.nu_min, r.nu_max, r.num_nu, out);
        default: return vag_flux_components4_batch(c, params, nb, r.t, r.nt, r.nu_min, r.nu_max, r.num_nu, out4);
    }
}

static void coalesce_serve(vag_ctx* c, std::vector<CoalesceRequest*>& batch) {
    const int nb = (int)batch.size();
    CoalesceRequest& lead = *batch[0];
    const size_t len = lead.out_len();
    bool ok = false;
    if (nb > 1) try {
        std::vector<vag_model_params> params(nb);
        for (int i = 0; i < nb; ++i) params[i] = *batch[i]->p;
        const bool comps = (lead.kind & 4) != 0;
        bool want[4] = {!comps, false, false, false};
        if (comps)
            for (int q = 0; q < 4; ++q)
                for (int i = 0; i < nb; ++i) want[q] = want[q] || batch[i]->out4[q] != nullptr;
        std::vector<double> buf[4];
        double* o4[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int q = 0; q < 4; ++q)
            if (want[q]) {
                buf[q].resize((size_t)nb * len);
                o4[q] = buf[q].data();
            }
        const int rc = coalesce_run_one(c, lead, params.data(), nb, o4[0], o4);
        if (rc == VAG_OK) {
            for (int i = 0; i < nb; ++i) {
                if (comps) {
                    for (int q = 0; q < 4; ++q)
                        if (batch[i]->out4[q]) std::memcpy(batch[i]->out4[q], o4[q] + (size_t)i * len, sizeof(double) * len);
                } else {
                    std::memcpy(batch[i]->out, o4[0] + (size_t)i * len, sizeof(double) * len);
                }
                batch[i]->rc = VAG_OK;
            }
            ok = true;
        }
    } catch (const std::exception&) {
        // the staging buffers could not be allocated: no exception crosses the C ABI -- the members are served one by one below,
        // straight into their own buffers (that path allocates nothing on the host)
        ok = false;
    }
    if (!ok)  // alone, or the batch failed as a whole: every member on its own, with its own error
        for (int i = 0; i < nb; ++i) {
            CoalesceRequest& r = *batch[i];
            r.rc = coalesce_run_one(c, r, r.p, 1, r.out, r.out4);
            if (r.rc) r.err = g_err;
        }
}

static int coalesce_submit(vag_ctx* c, CoalesceRequest& req) {
    std::unique_lock<std::mutex> lk(c->co_mutex);
    c->co_queue.push_back(&req);
    ++c->co_calls;
    if (!c->co_leader) {
        c->co_leader = true;
    } else {
        c->co_cv.notify_one();  // (the leader counts the queue)
        req.cv.wait(lk, [&] { return req.done || req.promoted; });
        if (req.done) {
            if (req.rc) g_err = req.err;
            return req.rc;
        }
        // promoted: this request heads the next batch
    }
    {   // the leader waits up to co_wait_us for company (callers of a pool arrive one interpreter hand-off apart)
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(c->co_wait_us);
        while ((int)c->co_queue.size() < c->co_max_batch && c->co_cv.wait_until(lk, deadline) != std::cv_status::timeout) {
        }
    }
    // the leader's batch: its own request and every queued one that asks the same thing, in arrival order
    std::vector<CoalesceRequest*> batch{&req};
    std::vector<CoalesceRequest*> rest;
    for (CoalesceRequest* r : c->co_queue) {
        if (r == &req) continue;
        if ((int)batch.size() < c->co_max_batch && r->same_request(req))
            batch.push_back(r);
        else
            rest.push_back(r);
    }
    c->co_queue.swap(rest);
    ++c->co_batches;
    lk.unlock();
    coalesce_serve(c, batch);  // (takes the context lock inside the entry points)
    lk.lock();
    for (CoalesceRequest* r : batch)
        if (r != &req) {
            r->done = true;
            r->cv.notify_one();  // (under the mutex: the member cannot return -- and its request leave the stack -- before this)
        }
    if (!c->co_queue.empty()) {
        c->co_queue.front()->promoted = true;  // stays the leader-in-waiting: co_leader remains set
        c->co_queue.front()->cv.notify_one();
    } else {
        c->co_leader = false;
    }
    lk.unlock();
    if (req.rc) g_err = req.err;
    return req.rc;
}

int vag_ctx_coalesce(vag_ctx* c, int max_batch, int wait_us) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (max_batch < 1 || wait_us < 0) return set_err(VAG_E_INVALID, "max_batch must be >= 1 and wait_us >= 0");
    std::lock_guard<std::mutex> lk(c->co_mutex);
    c->co_max_batch = max_batch;
    c->co_wait_us = wait_us;
    return VAG_OK;
}

int vag_ctx_coalesce_stats(vag_ctx* c, long long* calls, long long* batches) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    std::lock_guard<std::mutex> lk(c->co_mutex);
    if (calls) *calls = c->co_calls;
    if (batches) *batches = c->co_batches;
    return VAG_OK;
}

int vag_flux_density_grid_coalesced(vag_ctx* c, const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, double* out,
                                    double* const* out4) {
    if (!c || !p || !t || !nu || (!out && !out4)) return set_err(VAG_E_INVALID, "null context, model or buffer");
    if (nt <= 0 || nnu <= 0) return set_err(VAG_E_INVALID, "time and frequency arrays must be non-empty");
    CoalesceRequest r{out4 ? 4 : 0, p, t, nu, nt, nnu, 0, 0, 0, out, out4};
    return coalesce_submit(c, r);
}

int vag_flux_density_coalesced(vag_ctx* c, const vag_model_params* p, const double* t, const double* nu, int n, double* out,
                               double* const* out4) {
    if (!c || !p || !t || !nu || (!out && !out4)) return set_err(VAG_E_INVALID, "null context, model or buffer");
    if (n <= 0) return set_err(VAG_E_INVALID, "time array must be non-empty");
    CoalesceRequest r{out4 ? 5 : 1, p, t, nu, n, n, 0, 0, 0, out, out4};
    return coalesce_submit(c, r);
}

int vag_flux_coalesced(vag_ctx* c, const vag_model_params* p, const double* t, int nt, double nu_min, double nu_max, int num_nu, double* out,
                       double* const* out4) {
    if (!c || !p || !t || (!out && !out4)) return set_err(VAG_E_INVALID, "null context, model or buffer");
    if (nt <= 0) return set_err(VAG_E_INVALID, "time array must be non-empty");
    CoalesceRequest r{out4 ? 6 : 2, p, t, nullptr, nt, 0, nu_min, nu_max, num_nu, out, out4};
    return coalesce_submit(c, r);
}


static int details_impl(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, vag_details_shape* shape,
                        const vag_details_out* out, bool want_rvs) {
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (!params || !shape) return set_err(VAG_E_INVALID, "null model or shape");
    if (want_rvs && !(params->flags & VAG_FLAG_RVS)) return set_err(VAG_E_INVALID, "model has no reverse shock");
    const char* msg = validate_msg(params);
    if (msg) return set_err(VAG_E_INVALID, "%s", msg);
    if (!(t_min > 0) || !(t_max >= t_min)) return set_err(VAG_E_INVALID, "need 0 < t_min <= t_max");
    HIPCHK(hipSetDevice(c->device));
    if (c->d_params.ensure(sizeof(vag_model_params))) return VAG_E_HIP;
    if (c->d_tminmax.ensure(sizeof(double) * 2)) return VAG_E_HIP;
    const double tmm[2] = {t_min, t_max};
    HIPCHK(hipMemcpyAsync(c->d_params.p, params, sizeof(vag_model_params), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_tminmax.p, tmm, sizeof tmm, hipMemcpyHostToDevice, c->stream));
    int rc = run_model_stages(c, c->d_params.as<vag_model_params>(), 1, true);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    rc = check_status(c, 1);
    if (rc) return rc;
    if (fetch_meta(c)) return VAG_E_HIP;
    const VagGridMeta M = c->h_meta.as<VagGridMeta>()[0];
    shape->n_phi = M.n_phi;
    shape->n_theta = M.n_theta;
    shape->n_t = M.n_t;
    shape->n_reps = M.rep_phi_stride ? M.n_theta : M.n_reps;  // ((phi, theta) pair rows: the arrays below are the phi[0] slice)
    shape->symmetry = M.symmetry;
    shape->phi_mirrored = M.phi_mirrored;
    if (!out) return VAG_OK;
    const int nth = M.n_theta, nt = M.n_t;
    if (vag_hook("VAG_DEBUG_ROWS")) {  // developer aid: ODE status (and injection cutoff) per representative row
        std::vector<int> st(c->n_rows), inj(c->n_rows, -1);
        HIPCHK(hipMemcpy(st.data(), c->d_row_status.p, sizeof(int) * c->n_rows, hipMemcpyDeviceToHost));
        if (params->flags & VAG_FLAG_RVS) HIPCHK(hipMemcpy(inj.data(), c->d_inj.p, sizeof(int) * c->n_rows, hipMemcpyDeviceToHost));
        for (int r = 0; r < c->n_rows; ++r) std::fprintf(stderr, "row %d status %d inj %d\n", r, st[r], inj[r]);
    }
    std::vector<double> theta(nth), buf((size_t)c->n_cells * VAG_NSHOCK);
    std::vector<int> rep_of(nth);
    HIPCHK(hipMemcpy(theta.data(), c->d_theta.p, sizeof(double) * nth, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rep_of.data(), c->d_rep_of.p, sizeof(int) * nth, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(buf.data(), want_rvs ? c->d_shock_r.p : c->d_shock.p, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
    if (out->phi) HIPCHK(hipMemcpy(out->phi, c->d_phi.p, sizeof(double) * M.n_phi, hipMemcpyDeviceToHost));
    if (out->theta) std::memcpy(out->theta, theta.data(), sizeof(double) * nth);
    // Shock::broadcast_groups (src/dynamics/shock.cpp:42-91): every theta row shows its representative's state
    auto expand = [&](double* dst, int which, double scale) {
        if (!dst) return;
        const double* src = buf.data() + (size_t)which * c->n_cells;
        for (int j = 0; j < nth; ++j)
            for (int k = 0; k < nt; ++k) dst[(size_t)j * nt + k] = src[(size_t)rep_of[j] * nt + k] * scale;
    };
    expand(out->t_src, VS_TENG, 1 / U_SEC);
    expand(out->Gamma, VS_GAMMA, 1);
    expand(out->r, VS_R, 1 / U_CM);
    expand(out->t_comv, VS_TCOMV, 1 / U_SEC);
    expand(out->B, VS_B, 1 / U_GAUSS);
    expand(out->N_p, VS_NP, 1);
    expand(out->Gamma_th, VS_GAMMA_TH, 1);
    return VAG_OK;
}

int vag_details(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, vag_details_shape* shape,
                const vag_details_out* out) {
    ApiLock api_lock(c);
    return details_impl(c, params, t_min, t_max, shape, out, false);
}

int vag_profile_eval(vag_ctx* c, const vag_model_params* params, int kind, const double* x, int n, double* out) {
    ApiLock api_lock(c);
    if (!c) return set_err(VAG_E_INVALID, "null context");
    if (kind < 0 || kind > 2) return set_err(VAG_E_INVALID, "profile kind must be 0 (E_iso), 1 (Gamma0) or 2 (rho)");
    if (n <= 0 || !x || !out) return set_err(VAG_E_INVALID, "empty abscissa array");
    const char* msg = validate_msg(params);
    if (msg) return set_err(VAG_E_INVALID, "%s", msg);
    HIPCHK(hipSetDevice(c->device));
    if (c->d_params.ensure(sizeof(vag_model_params))) return VAG_E_HIP;
    DevBuf tmp;
    if (tmp.ensure(sizeof(double) * 2 * (size_t)n)) return VAG_E_HIP;
    double* d_x = tmp.as<double>();
    hipError_t e = hipMemcpyAsync(c->d_params.p, params, sizeof(vag_model_params), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_x, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(vag_profile_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_params.as<vag_model_params>(),
                           kind, d_x, n, d_x + n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_x + n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    tmp.release();
    if (e != hipSuccess) return set_err(VAG_E_HIP, "profile evaluation failed: %s", hipGetErrorString(e));
    return VAG_OK;
}

int vag_details_eat(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, int* n_phi_eff, double* t_obs,
                    double* doppler) {
    ApiLock api_lock(c);
    vag_details_shape sh;
    int rc = details_impl(c, params, t_min, t_max, &sh, nullptr, false);
    if (rc) return rc;
    if (fetch_meta(c)) return VAG_E_HIP;
    const VagGridMeta M = c->h_meta.as<VagGridMeta>()[0];
    if (n_phi_eff) *n_phi_eff = M.n_phi_eff;
    if (!t_obs && !doppler) return VAG_OK;  // shape query
    if (!t_obs || !doppler) return set_err(VAG_E_INVALID, "t_obs and doppler must be given together");
    const size_t total = (size_t)M.n_phi_eff * M.n_theta * M.n_t;
    DevBuf tmp;
    if (tmp.ensure(sizeof(double) * 2 * total)) return VAG_E_HIP;
    double* d_t = tmp.as<double>();
    hipLaunchKernelGGL(vag_eat_details_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream,
                       c->d_params.as<vag_model_params>(), c->d_meta.as<VagGridMeta>(), c->d_theta.as<double>(),
                       c->d_phi.as<double>(), c->d_rep_of.as<int>(), c->d_cellpar.as<double>(),
                       (params->flags & VAG_FLAG_SPREADING) ? c->d_shock.as<double>() + (size_t)VS_THETA * c->n_cells : nullptr, d_t,
                       d_t + total);
    if (hipGetLastError() != hipSuccess) {
        tmp.release();
        return set_err(VAG_E_HIP, "vag_eat_details_kernel launch failed");
    }
    hipError_t e1 = hipMemcpyAsync(t_obs, d_t, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipMemcpyAsync(doppler, d_t + total, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    tmp.release();
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return set_err(VAG_E_HIP, "copying the EAT details failed");
    return VAG_OK;
}

int vag_details_radiation(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, int rvs, double* const* arrays) {
    ApiLock api_lock(c);
    vag_details_shape sh;
    int rc = details_impl(c, params, t_min, t_max, &sh, nullptr, rvs != 0);  // runs the stages with the electron arrays kept
    if (rc) return rc;
    if (!arrays) return set_err(VAG_E_INVALID, "arrays must not be null");
    const int nth = sh.n_theta, nt = sh.n_t;
    const long long cells = c->n_cells;
    std::vector<double> buf((size_t)cells * 11), th((size_t)cells, 0.0);
    std::vector<int> rep_of(nth);
    const DevBuf& det = rvs ? c->d_celldet_r : c->d_celldet;
    const DevBuf& shock = rvs ? c->d_shock_r : c->d_shock;
    HIPCHK(hipMemcpy(buf.data(), det.p, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rep_of.data(), c->d_rep_of.p, sizeof(int) * nth, hipMemcpyDeviceToHost));
    const bool per_cell_theta = (params->flags & VAG_FLAG_SPREADING) != 0;
    if (per_cell_theta)
        HIPCHK(hipMemcpy(th.data(), static_cast<const double*>(shock.p) + (size_t)VS_THETA * cells, sizeof(double) * cells,
                         hipMemcpyDeviceToHost));
    std::vector<double> theta(nth);
    HIPCHK(hipMemcpy(theta.data(), c->d_theta.p, sizeof(double) * nth, hipMemcpyDeviceToHost));
    // VD_* rows: gamma_m, gamma_c, gamma_a, gamma_M, N_e, column_den, nu_m, nu_c, nu_a, nu_M, I_nu_max (code units)
    const int src_row[10] = {0, 1, 2, 3, 4, 6, 7, 8, 9, 10};
    const double scale[10] = {1, 1, 1, 1, 1, 1 / U_HZ, 1 / U_HZ, 1 / U_HZ, 1 / U_HZ, 1 / U_FLUX_DEN_CGS};
    for (int a = 0; a < 10; ++a) {
        if (!arrays[a]) continue;
        const double* src = buf.data() + (size_t)src_row[a] * cells;
        for (int j = 0; j < nth; ++j)
            for (int k = 0; k < nt; ++k) arrays[a][(size_t)j * nt + k] = src[(size_t)rep_of[j] * nt + k] * scale[a];
    }
    if (arrays[10])  // ShockDetails.theta: the evolved polar angle of a spreading jet, the grid angle otherwise
        for (int j = 0; j < nth; ++j)
            for (int k = 0; k < nt; ++k)
                arrays[10][(size_t)j * nt + k] = (params->flags & VAG_FLAG_SPREADING) ? th[(size_t)rep_of[j] * nt + k] : theta[j];
    return VAG_OK;
}

// SynElectrons::regime of every (theta, t) cell (determine_regime, synchrotron.cpp:45-60: the ordering of gamma_a, gamma_c, gamma_m,
// 1 ... 6, 0 = none), an integer the reference's parity contract covers exactly: from the electron rows the stages left -- and, where
// the SSC stages ran, checked against the tag vag_photons_ic_kernel stored for its IC kernels (VD_REGIME).
int vag_details_regime(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, int rvs, int32_t* regime) {
    ApiLock api_lock(c);
    vag_details_shape sh;
    int rc = details_impl(c, params, t_min, t_max, &sh, nullptr, rvs != 0);
    if (rc) return rc;
    if (!regime) return set_err(VAG_E_INVALID, "regime must not be null");
    const int nth = sh.n_theta, nt = sh.n_t;
    const long long cells = c->n_cells;
    std::vector<double> buf((size_t)cells * VAG_NDET);
    std::vector<int> rep_of(nth);
    const DevBuf& det = rvs ? c->d_celldet_r : c->d_celldet;
    HIPCHK(hipMemcpy(buf.data(), det.p, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rep_of.data(), c->d_rep_of.p, sizeof(int) * nth, hipMemcpyDeviceToHost));
    const bool ssc = rvs ? (params->flags & VAG_FLAG_RVS_SSC) != 0 : (params->flags & VAG_FLAG_SSC) != 0;
    auto order = [](double a, double cc, double m) {  // determine_regime
        if (a <= m && m <= cc) return 1;
        if (m <= a && a <= cc) return 2;
        if (a <= cc && cc <= m) return 3;
        if (cc <= a && a <= m) return 4;
        if (m <= cc && cc <= a) return 5;
        if (cc <= m && m <= a) return 6;
        return 0;
    };
    for (int j = 0; j < nth; ++j)
        for (int k = 0; k < nt; ++k) {
            const size_t q = (size_t)rep_of[j] * nt + k;
            const int tag = order(buf[(size_t)VD_GAMMA_A * cells + q], buf[(size_t)VD_GAMMA_C * cells + q], buf[(size_t)VD_GAMMA_M * cells + q]);
            if (ssc && tag != (int)buf[(size_t)VD_REGIME * cells + q])
                return set_err(VAG_E_INTERNAL, "cell (%d, %d): the regime tag of the IC kernels (%d) is not the ordering of the stored electrons (%d)",
                               j, k, (int)buf[(size_t)VD_REGIME * cells + q], tag);
            regime[(size_t)j * nt + k] = tag;
        }
    return VAG_OK;
}

int vag_details_rvs(vag_ctx* c, const vag_model_params* params, double t_min, double t_max, vag_details_shape* shape,
                    const vag_details_out* out) {
    ApiLock api_lock(c);
    return details_impl(c, params, t_min, t_max, shape, out, true);
}

}  // extern "C"
