/*
 * vegasafterglow_amd.h -- C-ABI of the MI355X-native afterglow forward-model engine.
 *
 * This is the drop-in boundary for ONE path of VegasAfterglow: the forward-shock
 * synchrotron light-curve model behind Model.flux_density_grid / Model.flux_density /
 * Model.flux and the per-walker log-likelihood built on it.  Every entry point states
 * the reference interface (file:line under the VegasAfterglow tree) it replaces.
 *
 * Conventions
 *  - plain C, no exceptions cross the ABI: every call returns 0 on success or a negative
 *    VAG_E_* code; vag_last_error() returns a thread-local message for the last failure.
 *  - all physical inputs are in the reference's user units (CGS: erg, cm, s, Hz, rad);
 *    flux densities come back in erg cm^-2 s^-1 Hz^-1, band fluxes in erg cm^-2 s^-1
 *    (pybind/pymodel.cpp:368-371,506-508).
 *  - the *_dev entry points take DEVICE pointers (HBM resident inputs/outputs) and are
 *    ordered on the context's HIP stream.  They are not fire-and-forget: the host waits
 *    (spinning on a pinned, coherent summary the grid kernel's last wavefront publishes --
 *    no copy, no stream synchronisation) for the batch's layout before it can size the
 *    later launches, and returns with those launches queued; results are complete when
 *    the stream reaches that point.  The host-pointer forms stage through the context's
 *    buffers and synchronise before returning.
 *  - there is no CPU fallback: without a HIP device vag_ctx_create fails with
 *    VAG_E_NO_DEVICE.
 */
#ifndef VEGASAFTERGLOW_AMD_H
#define VEGASAFTERGLOW_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAG_ABI_VERSION 13  /* v13: ticketed sharded calls (vag_loglike_shard_begin_dev / _end_dev); v12: vag_plan.n_ssc_slow_cells; v11: vag_plan.ode_rhs; a likelihood call's work tallies under vag_ctx_count_work (v10: VAG_E_INTERNAL; vag_ctx_set_stream orders the context's buffers across a change of stream) */

/* error codes */
#define VAG_OK 0
#define VAG_E_INVALID (-1)   /* bad argument: the reference raises ValueError (pybind/error_handling.h:31-69) */
#define VAG_E_NO_DEVICE (-2) /* no HIP device / HIP runtime failure at context creation */
#define VAG_E_HIP (-3)       /* a HIP call failed; message carries hipGetErrorString */
#define VAG_E_UNSUPPORTED (-4) /* configuration outside the accelerated path (today: a likelihood batch whose models differ in their flags) */
#define VAG_E_CAPACITY (-5)  /* grid larger than the engine's static limits */
#define VAG_E_NUMERIC (-6)   /* an ODE row could not find a step size (the reference throws odeint's step_adjustment_error) */
#define VAG_E_INTERNAL (-7)  /* an invariant of the engine failed (a defect, reported instead of a silently wrong flux) */

/* jet profiles: src/environment/jet.h:84-259 (TophatJet, GaussianJet, PowerLawJet),
 * math::two_component jet.h:421-437 via PyTwoComponentJet pybind/pymodel.cpp:130-146 */
#define VAG_JET_TOPHAT 0
#define VAG_JET_GAUSSIAN 1
#define VAG_JET_POWERLAW 2
#define VAG_JET_TWO_COMPONENT 3
/* Top-hat profile on the generic Ejecta with a constant magnetisation sigma0 (eps = E_iso, Gamma0 for theta <= theta_c):
 * the jet of the reference's tophat_sigma*_rs goldens (tests/python/golden/regenerate.py:141-149). */
#define VAG_JET_MAGNETIZED_TOPHAT 4
/* StepPowerLawJet(theta_c, E_iso, Gamma0, E_iso_w, Gamma0_w, k_e, k_g) and PowerLawWing(theta_c, E_iso_w, Gamma0_w, k_e, k_g):
 * pybind/pymodel.cpp:90-125, src/environment/jet.h:403-429 */
#define VAG_JET_STEP_POWERLAW 5
#define VAG_JET_POWERLAW_WING 6

/* Radiation flags.  VAG_FLAG_SSC / VAG_FLAG_KN = fwd_rad Radiation(ssc=, kn=): inverse-Compton cooling + SSC emission
 * (src/radiation/inverse-compton.*).  VAG_FLAG_RVS = Model(rvs_rad=Radiation(...)) i.e. the coupled forward+reverse
 * shock solve (src/dynamics/reverse-shock.tpp); VAG_FLAG_RVS_SSC / VAG_FLAG_RVS_KN = rvs_rad's ssc / kn. */
#define VAG_FLAG_SSC 1
#define VAG_FLAG_KN 2
#define VAG_FLAG_RVS 4
#define VAG_FLAG_RVS_SSC 8
#define VAG_FLAG_RVS_KN 16
/* jet(..., spreading=True): lateral expansion of the forward shock (forward-shock.tpp:36-40,78-84,110-116), per-row time
 * lattices and per-cell solid angles (observer.cpp:51-141). */
#define VAG_FLAG_SPREADING 32
/* jet(..., magnetar=Magnetar(L0, t0, q)): energy injection L0 (1 + t/t0)^-q inside theta_c (src/environment/jet.h:518-527,
 * pybind/pymodel.cpp:38-45); the jet then runs on the generic Ejecta profile forms of the reference. */
#define VAG_FLAG_MAGNETAR 64
/* Model(..., axisymmetric=False): full-circle phi grid, no mirror / on-axis shortcut (grid-refinement.h:671-689,
 * observer.cpp:215-222).  The named jets stay phi-independent, so every phi slice of the dynamics is the same solve. */
#define VAG_FLAG_NON_AXISYMMETRIC 128

/* media: src/environment/medium.h:50-133 (ISM, Wind with k_m = 2) */
#define VAG_MEDIUM_ISM 0
#define VAG_MEDIUM_WIND 1

/*
 * One forward model = the arguments of
 *   Model(jet, medium, Observer(lumi_dist, z, theta_obs), Radiation(eps_e, eps_B, p, xi_e),
 *         resolutions=(phi, theta, t), rtol, axisymmetric=True, radiative_fireball)
 * (pybind/pybind.cpp:384-422, pybind/pymodel.h:613-649), flattened to plain scalars.
 * All doubles; the two tags are int32.  Layout is fixed (272 bytes) and is what the
 * device kernels read straight from HBM.
 */
typedef struct vag_model_params {
    int32_t jet_type;    /* VAG_JET_* */
    int32_t medium_type; /* VAG_MEDIUM_* */
    /* jet (unused fields ignored by the profile) */
    double theta_c;  /* core half-opening angle [rad] */
    double E_iso;    /* isotropic-equivalent energy (core) [erg] */
    double Gamma0;   /* initial Lorentz factor (core) */
    double k_e;      /* PowerLawJet energy index */
    double k_g;      /* PowerLawJet Lorentz-factor index */
    double theta_w;  /* TwoComponentJet wing angle [rad] */
    double E_iso_w;  /* TwoComponentJet wing energy [erg] */
    double Gamma0_w; /* TwoComponentJet wing Lorentz factor */
    double duration; /* engine duration T0 [s] (shapes the reverse shock and its time lattice) */
    /* medium */
    double n_ism;  /* ISM number density [cm^-3]; Wind: ISM floor */
    double A_star; /* Wind parameter */
    double n0;     /* Wind inner plateau density [cm^-3]; +inf = none */
    /* observer */
    double lumi_dist; /* [cm] */
    double z;
    double theta_obs; /* [rad] */
    /* forward-shock radiation */
    double eps_e;
    double eps_B;
    double p;
    double xi_e;
    /* numerics */
    double phi_resol;   /* points per degree */
    double theta_resol; /* points per degree */
    double t_resol;     /* points per decade */
    double rtol;        /* ODE tolerance, (0,1) */
    int32_t radiative_fireball; /* 1 = radiative losses feed back on dynamics (default) */
    int32_t flags;              /* VAG_FLAG_* (Radiation(ssc=, kn=), pybind/pybind.cpp:368-377); other bits must be 0 */
    /* reverse-shock radiation (Model(rvs_rad=...), pybind/pymodel.h:613-629); read only when VAG_FLAG_RVS is set */
    double rvs_eps_e;
    double rvs_eps_B;
    double rvs_p;
    double rvs_xi_e;
    double sigma0; /* ejecta magnetisation, VAG_JET_MAGNETIZED_TOPHAT only (Ejecta(sigma0=...), pybind/pybind.cpp:224-272) */
    double k_m;    /* Wind density slope rho ~ r^-k_m (pybind/pymodel.cpp:153-186); 2 = the analytic Wind class */
    /* Magnetar(L0 [erg/s], t0 [s], q), read only with VAG_FLAG_MAGNETAR (pybind/pymodel.h:34-54) */
    double mag_L0;
    double mag_t0;
    double mag_q;
} vag_model_params;

/* Fill a params struct with the reference's defaults: Radiation xi_e = 1,
 * resolutions (0.06, 0.15, 6) (src/config/simulation-defaults.h:58-68), rtol 1e-6,
 * duration 1 s, n0 = +inf, radiative_fireball = 1, k_e = k_g = 2. */
void vag_params_default(vag_model_params* p);

/* Validate one params struct exactly like the reference's factories and Model ctor
 * (pybind/pymodel.cpp:47-186, pybind/pymodel.h:205-260,613-649).  0 or VAG_E_INVALID. */
int vag_params_validate(const vag_model_params* p);

const char* vag_last_error(void);
const char* vag_version(void);
/* Developer / test hooks are VAG_* environment variables (DESIGN.md names them).  The library reads the process environment once, inside
 * the first API call, and never on a call path afterwards (ABI v13; a thread pool may drive one context while another thread calls
 * setenv).  A process that changes such a variable later -- the test-suite does -- calls this to have it read again; not to be called
 * while another thread is inside the library. */
void vag_reload_env_hooks(void);
int vag_abi_version(void);

/* Number of visible HIP devices (0 when none / runtime missing). */
int vag_device_count(void);

/* ABI v12: bytes of device memory the library holds in this process, over all contexts.  A context's buffers only grow, to what the
 * largest request so far needed (+25 %), and are freed by vag_ctx_destroy: in a sampler's loop the figure stops moving after the first
 * calls (tests/test_gpu_fullsize.py holds it to that). */
long long vag_device_bytes_in_use(void);

/* ---- engine context: one per (process, device); owns stream + workspace in HBM ---- */
typedef struct vag_ctx vag_ctx;

int vag_ctx_create(int device, vag_ctx** out);
void vag_ctx_destroy(vag_ctx* ctx);
/* Use an external HIP stream (hipStream_t passed as void*); NULL = the context's own (non-blocking) stream.
 * The legacy default stream has the handle 0 and cannot be told apart from NULL: pass VAG_STREAM_LEGACY_DEFAULT for it
 * (PyTorch's default `torch.cuda.current_stream()` IS that stream: its `.cuda_stream` is 0). */
#define VAG_STREAM_LEGACY_DEFAULT ((void*)1)
/* Stream lifetime (ABI v11): a caller-owned stream must stay alive for the duration of every engine call made on it; it may be destroyed
 * between calls, before it is handed back -- the engine never touches the stream it leaves (the hand-off event that orders the
 * context's scratch buffers across streams is recorded at the end of each device-resident call, while the stream is known to be
 * alive).  VAG_E_HIP if the new stream cannot be made to wait for that event. */
int vag_ctx_set_stream(vag_ctx* ctx, void* hip_stream);
/* The value vag_ctx_set_stream would take to select the stream the context is on now (NULL = its own): lets a caller that
 * borrows the context for one call on another stream put the previous one back (ABI v9). */
int vag_ctx_get_stream(vag_ctx* ctx, void** out);
int vag_ctx_synchronize(vag_ctx* ctx);

/* Static per-model capacity limits of the device grids (rows/time nodes). */
typedef struct vag_limits {
    int32_t max_theta; /* theta nodes per model */
    int32_t max_phi;   /* phi nodes per model */
    int32_t max_time;  /* time-lattice nodes per row */
    int32_t max_nu;    /* frequencies per launch (grids with more are chunked inside the engine; a band integrates at most this many) */
} vag_limits;
void vag_get_limits(vag_limits* out);

/*
 * Model.flux_density_grid(t[nt] ascending, nu[nnu]) -> total[nnu][nt]
 * (pybind/pybind.cpp:424, pybind/pymodel.cpp:498-514, src/core/observer.h:355-445),
 * batched over nb independent models sharing (t, nu).  out is [nb][nnu][nt] row-major.
 */
int vag_flux_density_grid_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt,
                                const double* nu, int nnu, double* out);

/* Same request with the components kept apart: out_sync = FluxDict.fwd.sync, out_ssc = FluxDict.fwd.ssc (zeros when
 * Radiation.ssc is off), each [nb][nnu][nt] (pybind/pybind.cpp:472-483).  nt * nnu <= 4096. */
int vag_flux_density_grid_components_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt,
                                           const double* nu, int nnu, double* out_sync, double* out_ssc);

/* All four FluxDict components {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} (pybind/pybind.cpp:472-483), each [nb][nnu][nt];
 * NULL entries of out4 are skipped, disabled components come back as zeros.  nt * nnu <= 4096. */
int vag_flux_density_grid_components4_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt,
                                            const double* nu, int nnu, double* const* out4);

/* Sky images (Model.sky_image; the engine's own definition, INTEGRATION.md -- not pinned to the reference's method of that name).
 * Added after VAG_ABI_VERSION 13 without changing it: callers detect vag_sky_image_batch / vag_sky_moments_batch by symbol.
 * Every (phi, theta) row's equal-arrival-time term of every (nu, t) -- the terms flux_density_grid sums, in the same units -- is
 * placed on the sky at X = r (cos theta sin theta_v - sin theta cos phi cos theta_v) / D_A, Y = r sin theta sin phi / D_A
 * [rad], D_A = d_L / (1 + z)^2, +X along the projected jet axis; log r interpolated like the term, phi spread over the row's
 * azimuthal bin in max(1, ceil(n_az dphi / 2 pi)) parts (both signs of phi on mirrored grids).
 * image [nb][nnu][nt][npixel][npixel], [iy][ix], pixel size fov / npixel, centred on the burst: a part goes to
 * ix = floor((X + fov / 2) / (fov / npixel)), likewise iy; parts outside the image are summed into outside [nb][nnu][nt] (NULL:
 * not wanted).  image.sum + outside = flux_density_grid up to summation order.  erg cm^-2 s^-1 Hz^-1 per pixel.
 * fov finite and > 0, 1 <= npixel <= 4096, n_az <= 0: 4 * npixel.  Results are bitwise reproducible run to run. */
int vag_sky_image_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                        double fov, int npixel, int n_az, double* image, double* outside);

/* Flux-weighted moments of the same point set before any pixelation, moments [nb][nnu][nt][6]: F (= flux_density_grid), centroid
 * Xbar, Ybar [rad], central second moments varX, varY, covXY [rad^2] (two passes: accurate for a centroid many widths off
 * centre).  F = 0: NaN for the five shape values.  n_az <= 0: 256. */
int vag_sky_moments_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                          int n_az, double* moments);

/* The same moments with the azimuthal integral done exactly (the n_az -> infinity limit of vag_sky_moments_batch): every row's
 * term is spread uniformly over its phi bin and its first and second moments there are taken in closed form, then the rows are
 * combined with Chan's pairwise update in a fixed order.  Same output layout and NaN rule as vag_sky_moments_batch; results are
 * bitwise reproducible and do not depend on the rest of the batch.  Added after VAG_ABI_VERSION 13 (detect by symbol). */
int vag_sky_centroid_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                           double* moments);

/* Complex visibilities of the same parts as vag_sky_moments_batch (a direct Fourier sum, no pixels).  Added after VAG_ABI_VERSION
 * 13 (detect by symbol).  Every part (w, X, Y) is placed on the sky as the centroid likelihood places a centroid, east = X sin pa +
 * Y cos pa, north = X cos pa - Y sin pa (pa [rad], no offset: a shift (east0, north0) multiplies V by
 * exp(-2 pi i (u east0 + v north0))), and V(u, v) = sum w exp(-2 pi i (u east + v north)), u east, v north, in wavelengths.
 * u, v [nnu][nt][nbl] are the baselines of every (nu, t) slot, shared by the batch; vis [nb][nnu][nt][nbl][2] (re, im), units of
 * vag_flux_density_grid_batch, so V(0, 0) is the grid flux up to summation order.  1 <= nbl <= VAG_SKY_MAX_BASELINES, u, v and pa
 * finite, n_az <= 0: 1024.  Results are bitwise reproducible and do not depend on the rest of the batch. */
#define VAG_SKY_MAX_BASELINES 65536
int vag_sky_visibility_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu, int nnu,
                             const double* u, const double* v, int nbl, double pa, int n_az, double* vis);

/* Linear polarization of the same parts ("Polarization"; the engine's own definition).  Added after
 * VAG_ABI_VERSION 13 (detect by symbol).  A random magnetic field, axially symmetric about the shock normal (taken as the radial
 * direction), of anisotropy b = 2 <B_par^2> / <B_perp^2> (0: in the shock plane, 1: isotropic): a part seen at the fluid-frame
 * angle theta' from the normal, s = sin^2 theta' = (1 - mu^2) / (Gamma - u mu)^2, is polarized by
 * Pi = pi_max (b - 1) s / (2 + (b - 1) s) along (Pi < 0) or across (Pi > 0) the projected normal psi = atan2(Y, X):
 * Q = -Pi w cos 2 psi, U = -Pi w sin 2 psi.  SSC passes are unpolarized.  Index 0: forward shock, 1: reverse shock; b finite and
 * >= 0; pi_max <= 1, pi_max < 0: (p + 1) / (p + 7/3) with that shock's own p.  One spec per model. */
typedef struct vag_pol_spec {
    double b[2];
    double pi_max[2];
} vag_pol_spec;

/* Integrated Stokes parameters, out [nb][nnu][nt][3]: I (= flux_density_grid up to summation order), Q, U on the sky with +X at
 * position angle pa [rad] east of north: Q_sky = Q cos 2pa - U sin 2pa, U_sky = Q sin 2pa + U cos 2pa, so 1/2 atan2(U, Q) is the
 * IAU polarization angle.  On a mirrored grid the jet-frame U is exactly 0.  n_az <= 0: 256.  Results are bitwise reproducible and
 * do not depend on the rest of the batch. */
int vag_sky_polarization_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu,
                               int nnu, const vag_pol_spec* pol, double pa, int n_az, double* out);

/* Stokes maps on the pixel grid of vag_sky_image_batch, in the jet frame: image [nb][nnu][nt][3][npixel][npixel] (I, Q, U; the I
 * map is bit for bit vag_sky_image_batch's image), outside [nb][nnu][nt][3] (NULL: not wanted) the Stokes sums of the parts outside
 * the image.  fov, npixel, n_az as vag_sky_image_batch. */
int vag_sky_stokes_image_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, const double* nu,
                               int nnu, const vag_pol_spec* pol, double fov, int npixel, int n_az, double* image, double* outside);

/* Test-facing: evaluates device routine `fn` (VAG_MATH_*) of this library on n points, on the device, with the context's own
 * softplus / log2 tables.  in: [n][n_in(fn)], out: [n][n_out(fn)].  Added after VAG_ABI_VERSION 13 (detect by symbol).
 * n_in = n_out = 1 for the elementwise routines (the sp_fast forms take z and give log2(1 + 2^z)), except:
 *   VAG_MATH_SYN_CELL  in  {gamma_m, gamma_c, gamma_a, gamma_M, column_den, B, p, x0, x1} (internal units, x = log2 nu);
 *                      out {the VAG_NPAR block of syn_photons_build, log2_I_nu_fast on that block in registers at x0, x1, on it as a
 *                      strided column at x0, x1, log2_I_nu_fast2(x0, x1), the exact-libm log2_I_nu at x0, x1}: VAG_NPAR + 8;
 *   VAG_MATH_IC_CELL   in  {VAG_NPAR block, VAG_NQ IC extras, p, x0, x1}; out {log2_I_nu_ic, _straight, _pair, each at x0, x1};
 *   VAG_MATH_POISSON_DEVIANCE  in {N, mu}; out the Poisson deviance D(N, mu) (n_in = 2, n_out = 1);
 *   VAG_MATH_LOG_SLOPE  in {F_0 .. F_7, c_0 .. c_7, K}; out sum_{k = 1 .. K-1} c_k ln(F_k / F_0), NaN unless F_0 .. F_{K-1} are all
 *                      finite and > 0 (n_in = 17, n_out = 1; entries from K on are not read);
 *   VAG_MATH_ELEC_CELL in  {t_comv, r, Gamma_th, B, N_p, eps_e, p, xi_e, relic flag (0 / 1), inj.gamma_M, inj.gamma_m, inj.gamma_c}
 *                      (internal units; the inj electrons are read for a relic cell only): syn_cell with Gamma = 1, t_eng = 0;
 *                      out {gamma_m, gamma_c, gamma_a, gamma_M, N_e, column_den, nu_m, nu_c, nu_a, nu_M, I_nu_max} (n_in = 12, n_out = 11);
 *   VAG_MATH_FWD_STATE in  {Gamma, rho, U_th, m2, eps_B} (internal units): the shock state vag_cells_kernel finishes per cell;
 *                      out {Gamma_th, B, N_p, compression ratio} (n_in = 5, n_out = 4; m2 = 0, an unshocked cell, gives 1, 0, 0, 0);
 *   VAG_MATH_LDS_ADD   in  {slot, value}: the 64 lanes of a wavefront add their values into the slots (integers in [0, 64)) they
 *                      name with one ds_add_f64; out: slot `lane`'s total.
 * The reverse shock's closed forms and what turns the pair solver's state into cells (vag_rs.h; internal units):
 *   VAG_MATH_REL_GAMMA in  {g1, g2}; out {rel_Gamma, rel_Gamma_f} (n_in = 2, n_out = 2);
 *   VAG_MATH_SHOCK_JUMP in {gamma_rel, sigma}; out {downstr_4vel, jump_4vel, jump_4vel_f} (n_in = 2, n_out = 3);
 *   VAG_MATH_SOUND_SPEED in {G}; out {sound_speed, sound_speed_f} (n_in = 1, n_out = 2);
 *   VAG_MATH_RVS_STATE in  {Gamma, x4, x3, m3, U3, r, eps4, m4, Gamma4, eps_B, crossing flag (0 / 1), and the cross state the frozen
 *                      shell reads: V3_comv_x, rho3_x, B3_ordered_x}; out {Gamma_th, B, N_p of rvs_shock_state, then V3_comv, rho3,
 *                      B3_ordered of rvs_cross_state on the same state} (n_in = 14, n_out = 6);
 *   VAG_MATH_CROSS_LATTICE in {ts, t_end, t_dec, T0, t_num, base_t_num, k} (0 < ts < t_end, t_dec, T0 > 0, integers 2 <= t_num <= 4096,
 *                      1 <= base_t_num <= 4096, 0 <= k < t_num); out {node(k), n_pre, n_post, plain} (n_in = 7, n_out = 4);
 *   VAG_MATH_RVS_EXTRAP in {16 nodes of (r, Gamma_th, B, N_p), inj (an integer in [0, 16])}: one lane runs rvs_early_extrap on the row;
 *                      out {the 16 (Gamma_th, B, N_p) after the call} (n_in = 65, n_out = 48);
 *   VAG_MATH_PAIR_INIT in  {Gamma4 (> 1), deps0_dt, dm0_dt, T0 (> 0), t0 (> 0), eps_e_th, medium type (VAG_MEDIUM_ISM, or VAG_MEDIUM_WIND
 *                      with k = 2), rho_ism, A, r02}; out the 11 entries of PairShock::init_state in state order: Gamma, x4, x3, m2, m3,
 *                      U2, U3, r, t_comv, eps4, m4 (n_in = 10, n_out = 11).
 * The inverse-Compton routines below vag_ic_photon_kernel: the tables, Y(gamma), the cooling fixed points (vag_ic.h, vag_ic_kernels.h;
 * internal units):
 *   VAG_MATH_KN_LUT    in  {k (an integer in [0, 128))}; out {ratio, log2 ratio} of node k of the context's Klein-Nishina table, as
 *                      vag_ctx_create filled it on the host (n_in = 1, n_out = 2);
 *   VAG_MATH_KN_CORR   in  {lg2_nu, lg2_x}; out {corr, lg2_corr} of compton_correction_pair_lg2(lg2_nu), then {corr, lg2_corr} of
 *                      compton_correction_pair_node(lg2_x, exp2(lg2_x)), both on that table; a NaN lg2_x stands for the
 *                      argument the first form makes of lg2_nu itself, lg2_nu + log2(h / (m_e c^2)) (n_in = 2, n_out = 4);
 *   VAG_MATH_IC_TABLE  in  {n (an integer in [-1, 16]), first, th_min, th_max, x, 16 table words}: ic_table_eval_hdr on the row's own
 *                      words with last = first + 2 IC_Q (n - 1); out {value, breach bits} (n_in = 21, n_out = 2; words from n on are
 *                      never used: for n < 2 words 0 and 1 are still loaded and the result discarded, so no index past the
 *                      table is formed only for n >= 2);
 *   VAG_MATH_IC_BIN_INTEGRAL in {f_lo, f_hi, nu_lo, nu_hi, lg2f_lo, lg2f_hi, lg2r, inv_lg2r, trap}; out power_law_bin_integral of
 *                      them as given (n_in = 9, n_out = 1);
 *   VAG_MATH_IC_SUFFIX_SCAN in {the lane's four words}: the 256 words of a wavefront go through suffix_scan4 in LDS; out word d is
 *                      the sum of the wavefront's words from d on (n_in = 4, n_out = 4; a wave routine);
 *   VAG_MATH_IC_COLUMN_DEN in {gamma, gamma_m, gamma_c, gamma_M, p, regime (an integer in [0, 6]), column_den, Y_c, Y(gamma)}; out
 *                      electron_column_den (n_in = 9, n_out = 1);
 *   VAG_MATH_IC_Y      in  {gamma_m, gamma_c, p, B, Y_T, Klein-Nishina flag (0 / 1), g0, g1, nu0, nu1}: IcY::init; out {gamma_m_hat,
 *                      gamma_c_hat, gamma_self, regime, number of segments, the three (slope, lg2_lower, lg2_const) as icy_store writes
 *                      them (0, inf, 0 past the number of segments), Y(gamma = g0), Y(g1), Y(nu0), Y(nu1)} (n_in = 10, n_out = 18);
 *   VAG_MATH_IC_STEP   in  {t_comv, B, gamma_m, gamma_c, p, eps_e / eps_B, Klein-Nishina flag, gamma_M}: one pass of the body of
 *                      gamma_c's fixed point at gamma_c and of gamma_M's at gamma_M; out {Y_T, Y(gamma_c), the next gamma_c,
 *                      gamma_M_of(B, Y(gamma_c)), gamma_M_of(B, Y(gamma_M))} (n_in = 8, n_out = 5);
 *   VAG_MATH_IC_FIXED_POINT in {t_comv, B, gamma_m, the cell's own gamma_c, the previous cell's cooled gamma_c, p, eps_e / eps_B,
 *                      Klein-Nishina flag, the gamma_M to start from}: ic_gamma_c_cell, then ic_gamma_M on the Y(gamma) it leaves;
 *                      out {gamma_c, the gamma_c its Y(gamma) is built for, Y_T, passes, gamma_M, passes} (n_in = 9, n_out = 6);
 *   VAG_MATH_IC_GAMMA_A in {B, column_den, gamma_m, gamma_c, the gamma_c Y(gamma) is built for, p, Y_T, Klein-Nishina flag, and three
 *                      numbers a, c, m}: IcY::init, Y_c = Y(gamma_c), syn_gamma_a_ic with syn_I_peak(B, column_den) and determine_regime
 *                      as vag_photons_ic_kernel calls them; out {gamma_a, Y_c, determine_regime(gamma_a, gamma_c, gamma_m),
 *                      determine_regime(a, c, m)} (n_in = 11, n_out = 4).
 * The wave routines (WAVE_PREFIX_SUM, WAVE_SUM, SKY_WAVE_SUM, LDS_ADD, IC_SUFFIX_SCAN) run one wavefront per 64 points and need n % 64 == 0.
 * 0, VAG_E_INVALID (unknown fn, n <= 0, a null pointer, n % 64 != 0 for a wave routine, a bad slot, a point outside the ranges stated
 * above: a flag that is not 0 or 1, t_num < 2, k outside the lattice, an unknown medium type, ...) or VAG_E_HIP. */
enum {
    VAG_MATH_EXP2_FAST = 0, VAG_MATH_EXP2_ODE, VAG_MATH_EXP2_SAT, VAG_MATH_EXP2_OR_ZERO,
    VAG_MATH_LOG2_FAST, VAG_MATH_LOG2_TAB, VAG_MATH_LOG2_TAB_NB,
    VAG_MATH_RCP_FAST, VAG_MATH_RCP_ODE, VAG_MATH_RCP1, VAG_MATH_SQRT_FAST, VAG_MATH_SQRT_ODE, VAG_MATH_SQRT1,
    VAG_MATH_SP_FAST, VAG_MATH_SP_FAST_GLOBAL, VAG_MATH_SP_FAST_SEL,
    VAG_MATH_SYN_CELL, VAG_MATH_IC_CELL,
    VAG_MATH_WAVE_PREFIX_SUM, VAG_MATH_WAVE_SUM, VAG_MATH_SKY_WAVE_SUM, VAG_MATH_LDS_ADD,
    VAG_MATH_LOG_NDTR, /* ln Phi(z) of the upper-limit term (vag_loglike_lim_batch) */
    VAG_MATH_POISSON_DEVIANCE, /* in {N, mu}, out D = mu - N - N ln(mu / N) (mu for N = 0) of the counts term (vag_loglike_counts_batch) */
    VAG_MATH_LOG_SLOPE, /* in {8 fluxes, 8 coefficients, K}, out the pivot-form log-slope of the spectral-index term (vag_loglike_index_batch) */
    VAG_MATH_ELEC_CELL, /* syn_cell: the electrons and break frequencies of one cell (vag_cells_kernel) */
    VAG_MATH_FWD_STATE, /* fwd_shock_state: Gamma_th, B, N_p of one forward-shock cell from the raw ODE state (vag_cells_kernel) */
    VAG_MATH_REL_GAMMA, VAG_MATH_SHOCK_JUMP, VAG_MATH_SOUND_SPEED, /* the reverse shock's closed forms, exact and fast (vag_rs.h) */
    VAG_MATH_RVS_STATE, /* rvs_shock_state and rvs_cross_state: the reverse-shock cell from the pair solver's state (vag_dynamics_pair_kernel) */
    VAG_MATH_CROSS_LATTICE, /* CrossLattice: one node and the integers of a row's refined time lattice */
    VAG_MATH_RVS_EXTRAP, /* rvs_early_extrap on one row of 16 nodes */
    VAG_MATH_PAIR_INIT, /* PairShock::init_state */
    VAG_MATH_KN_LUT, VAG_MATH_KN_CORR, /* the Klein-Nishina table of the context and its two look-ups (vag_ic.h) */
    VAG_MATH_IC_TABLE, /* ic_table_eval_hdr on a table carried in the row */
    VAG_MATH_IC_BIN_INTEGRAL, /* power_law_bin_integral */
    VAG_MATH_IC_SUFFIX_SCAN, /* suffix_scan4 over the 256 words of a wavefront */
    VAG_MATH_IC_COLUMN_DEN, /* electron_column_den */
    VAG_MATH_IC_Y, /* IcY::init and the Y(gamma) it builds */
    VAG_MATH_IC_STEP, /* one pass of the bodies of the gamma_c and gamma_M fixed points */
    VAG_MATH_IC_FIXED_POINT, /* ic_gamma_c_cell and ic_gamma_M: the loops vag_ic_cooling_kernel and vag_photons_ic_kernel run */
    VAG_MATH_IC_GAMMA_A, /* syn_gamma_a_ic and determine_regime */
    /* the split flux kernel's instruction forms of exp2_fast and sp_fast<true> (vag_device.h: exp2_fast_as, sp_fast with its magic number in
     * a vector register) and sp_fast<true> itself; one argument, one result each, on the domains of exp2_fast and sp_fast */
    VAG_MATH_EXP2_FAST_CHAIN, VAG_MATH_SP_FAST_RELU, VAG_MATH_SP_FAST_RELU_VMAGIC,
    VAG_MATH_COUNT
};
int vag_debug_device_math(vag_ctx* ctx, int fn, const double* in, int n, double* out);

/*
 * Model.flux_density(t[n] ascending, nu[n]) -> total[n]
 * (pybind/pybind.cpp:427, pybind/pymodel.cpp:373-389, src/core/observer.h:447-538),
 * batched: out is [nb][n].
 */
int vag_flux_density_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, const double* nu,
                           int n, double* out);
/* The same series with FluxDict's components apart (pymodel.cpp:373-389): out4[i] != NULL receives component i of
 * {fwd.sync, fwd.ssc, rvs.sync, rvs.ssc} as [nb][n]; components the model does not enable come back as zeros. */
int vag_flux_density_components4_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, const double* nu,
                                       int n, double* const* out4);

/*
 * Model.flux(t[nt], nu_min, nu_max, num_nu) -> band flux[nt]
 * (pybind/pybind.cpp:430, pybind/pymodel.cpp:391-410, src/core/observer.h:555-567,
 * Boole weights src/core/quadrature.h:153-196); out is [nb][nt].
 */
int vag_flux_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt, double nu_min,
                   double nu_max, int num_nu, double* out);
/* Same with the components apart: out_sync = fwd.sync, out_ssc = fwd.ssc, each [nb][nt]. */
int vag_flux_components_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt,
                              double nu_min, double nu_max, int num_nu, double* out_sync, double* out_ssc);
/* ... and all four components, each [nb][nt] (NULL entries skipped). */
int vag_flux_components4_batch(vag_ctx* ctx, const vag_model_params* params, int nb, const double* t, int nt,
                               double nu_min, double nu_max, int num_nu, double* const* out4);

/* Device-pointer forms: params/t/nu/out are HBM addresses; stream-ordered on the context stream (see the note at the top). */
int vag_flux_density_grid_batch_dev(vag_ctx* ctx, const vag_model_params* d_params, int nb, const double* d_t,
                                    int nt, const double* d_nu, int nnu, double* d_out);
int vag_flux_density_batch_dev(vag_ctx* ctx, const vag_model_params* d_params, int nb, const double* d_t,
                               const double* d_nu, int n, double* d_out);

/*
 * Batched log-likelihood: the seam emcee's vectorized log_prob_batch calls
 * (VegasAfterglow/fitting/samplers.py:61-91 -> fitter.py:503-533).
 *
 * Point data (sorted by time, weights normalised to sum N as in fitter.py:407-451):
 *   chi2 = sum_i w_i ((ln F_obs_i - ln max(F_mod_i, 1e-300)) / (err_i / F_obs_i))^2
 *   loglike = -0.5 chi2; non-finite chi2 -> -inf (samplers.py:61-70).
 * The transformer (fitting/utils.py:110-135) is expressed as a slot map: free
 * parameter d of theta writes field slot[d] (a VAG_P_* index) of a copy of `base`,
 * as 10**theta when is_log[d] != 0.
 */
#define VAG_P_THETA_C 0
#define VAG_P_E_ISO 1
#define VAG_P_GAMMA0 2
#define VAG_P_K_E 3
#define VAG_P_K_G 4
#define VAG_P_THETA_W 5
#define VAG_P_E_ISO_W 6
#define VAG_P_GAMMA0_W 7
#define VAG_P_DURATION 8
#define VAG_P_N_ISM 9
#define VAG_P_A_STAR 10
#define VAG_P_N0 11
#define VAG_P_LUMI_DIST 12
#define VAG_P_Z 13
#define VAG_P_THETA_OBS 14
#define VAG_P_EPS_E 15
#define VAG_P_EPS_B 16
#define VAG_P_P 17
#define VAG_P_XI_E 18
#define VAG_P_COUNT 19 /* slots 0..18 are contiguous; the reverse-shock radiation parameters follow the numerics block */
#define VAG_P_RVS_EPS_E 24
#define VAG_P_RVS_EPS_B 25
#define VAG_P_RVS_P 26
#define VAG_P_RVS_XI_E 27
#define VAG_P_SIGMA0 28
#define VAG_P_K_M 29
#define VAG_P_MAG_L0 30
#define VAG_P_MAG_T0 31
#define VAG_P_MAG_Q 32

/* Not a Model field: the host-galaxy extinction A_V of ModelParams (types.py:77).  A free parameter with this slot only
 * scales the point-data model fluxes by exp(-A_V * ext_kernel[i]) (fitter.py:512-519). */
#define VAG_P_A_V 1000

/* Not Model fields either: the sky placement of the centroid groups of vag_loglike_sky_batch and of the visibility groups of
 * vag_loglike_vis_batch (position angle of the projected jet axis +X, measured east of north [rad]; the burst's offset east and
 * north of the reference position [rad]).  Only those entry points accept them, with at least one such group. */
#define VAG_P_SKY_PA 1001
#define VAG_P_SKY_EAST0 1002
#define VAG_P_SKY_NORTH0 1003

/* Nor are these: the magnetic field behind the shocks as the polarization groups of vag_loglike_pol_batch see it (vag_pol_spec: the
 * anisotropy b and Pi_max of the forward shock, then of the reverse shock).  Only that entry point accepts them, with at least one
 * polarization group; VAG_P_SKY_PA is accepted there too. */
#define VAG_P_POL_B 1004
#define VAG_P_POL_PI_MAX 1005
#define VAG_P_POL_B_RVS 1006
#define VAG_P_POL_PI_MAX_RVS 1007

/* Nor are these: the fractional systematic s_g of noise group g of vag_loglike_noise_batch, g = 0 .. VAG_NOISE_MAX_GROUPS - 1.
 * Only that entry point accepts VAG_P_NOISE_SYS0 + g, and only when its vag_noise_fit_spec has group g (g < n_groups). */
#define VAG_P_NOISE_SYS0 1008
#define VAG_NOISE_MAX_GROUPS 8
/* Nor is this: the absorbing column N_H [cm^-2] of the count-spectrum groups of vag_loglike_fold_batch.  Only that entry point accepts
 * it, and only when some group carries a cross-section (vag_fold_obs::sigma). */
#define VAG_P_N_H 1016
/* Nor are these: the amplitude a_c of additive template c of vag_loglike_tmpl_batch, c = 0 .. VAG_TMPL_MAX - 1.  Only that entry point
 * accepts VAG_P_TMPL_AMP0 + c, and only when its vag_template_fit_spec has template c (c < n_templates). */
#define VAG_P_TMPL_AMP0 1017
#define VAG_TMPL_MAX 8
/* Nor are these: the outlier fraction P_g, the extra scatter b_g and the mean offset mu_g of robust noise group g of
 * vag_loglike_robust_batch, g = 0 .. VAG_NOISE_MAX_GROUPS - 1.  Only a request with a vag_robust_fit_spec accepts them, and only for a
 * group whose bit is set in its mask. */
#define VAG_P_ROBUST_FRAC0 1025
#define VAG_P_ROBUST_SCALE0 1033
#define VAG_P_ROBUST_SHIFT0 1041

/* One group of VLBI centroid positions at one frequency (added after VAG_ABI_VERSION 13, detect by symbol).  The model centroid
 * (Xbar, Ybar) of vag_sky_centroid_batch(t, nu) is placed on the sky as
 *   east = east0 + Xbar sin PA + Ybar cos PA,   north = north0 + Xbar cos PA - Ybar sin PA
 * (+X points at position angle PA, +Y at PA + 90 degrees, both measured from north through east; every named profile has Ybar = 0)
 * and adds sum_i weight_i [((east_i - east) / err_east_i)^2 + ((north_i - north) / err_north_i)^2] to the walker's chi^2. */
typedef struct vag_centroid_obs {
    double nu;                /* [Hz] */
    int32_t n;                /* epochs */
    int32_t pad;
    const double* t;          /* [n] ascending [s]: the group's own request (own grid from its own times) */
    const double* east;       /* [n] [rad] */
    const double* north;      /* [n] [rad] */
    const double* err_east;   /* [n] > 0 [rad] */
    const double* err_north;  /* [n] > 0 [rad] */
    const double* weight;     /* [n] */
} vag_centroid_obs;

typedef struct vag_sky_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_centroid_obs* groups;  /* [n_groups] */
    double pa_fixed, east0_fixed, north0_fixed; /* values of PA / east0 / north0 that are not free parameters [rad] */
} vag_sky_fit_spec;

/* One band-integrated data group of Fitter.add_flux (fitter.py:316-377): Model.flux(t, nu_min, nu_max, num_points) is
 * evaluated as its own request (own grid from its own time range), exactly like the reference's loop (fitter.py:524-531). */
typedef struct vag_band_obs {
    double nu_min, nu_max;  /* [Hz] */
    int32_t num_points;     /* Boole nodes across the band */
    int32_t n;              /* observations */
    const double* t;        /* [n] ascending [s] */
    const double* ln_flux;  /* [n] ln F_obs [erg/cm^2/s] */
    const double* ln_err;   /* [n] err / F_obs */
    const double* weight;   /* [n] */
} vag_band_obs;

typedef struct vag_fit_spec {
    vag_model_params base; /* fixed parameters + numerics */
    int32_t ndim;          /* number of free parameters (<= 16) */
    int32_t slot[16];      /* VAG_P_* target of each free parameter */
    int32_t is_log[16];    /* 1: value = 10**theta */
    int32_t n_data;        /* number of point observations (may be 0 when only band data is fitted) */
    int32_t pad;
    const double* t;        /* [n_data] observer times, ascending [s] */
    const double* nu;       /* [n_data] frequencies [Hz] */
    const double* ln_flux;  /* [n_data] ln F_obs */
    const double* ln_err;   /* [n_data] err/F_obs */
    const double* weight;   /* [n_data] normalised weights */
    /* ABI v6 */
    const double* ext_kernel;   /* [n_data] 0.4 ln10 k(lambda_rest) of the extinction law, or NULL (fitter.py:439-449) */
    double a_v_fixed;           /* A_V when it is not a free parameter (0 = no extinction) */
    int32_t n_bands;            /* band-integrated groups */
    int32_t pad2;
    const vag_band_obs* bands;  /* [n_bands] */
    /* ABI v7: the bounds mask and the priors of log_prob_batch (fitting/samplers.py:72-91) on the device.
     * use_priors = 0: the call returns ln L for every walker (ABI v6 behaviour).
     * use_priors = 1: a walker with any theta[d] outside [lower[d], upper[d]] is NOT evaluated and scores -inf; the others
     * score ln L + sum_d ln prior_d(theta[d]) with prior_kind[d] one of VAG_PRIOR_* acting on the SAMPLER-space value
     * (bilby.core.prior.Uniform / Gaussian / LogUniform.ln_prob; params.py:209-227 builds Uniform(lower, upper) by default). */
    int32_t use_priors;
    int32_t pad3;
    double lower[16], upper[16];
    int32_t prior_kind[16];
    double prior_a[16]; /* GAUSSIAN: mu;    LOG_UNIFORM: minimum (> 0); UNIFORM: unused (the bounds are the support) */
    double prior_b[16]; /* GAUSSIAN: sigma; LOG_UNIFORM: maximum */
} vag_fit_spec;
#define VAG_PRIOR_UNIFORM 0     /* -ln(upper - lower) */
#define VAG_PRIOR_GAUSSIAN 1    /* -(x - mu)^2 / (2 sigma^2) - ln(sigma sqrt(2 pi)) */
#define VAG_PRIOR_LOG_UNIFORM 2 /* -ln(x ln(max / min)) for min <= x <= max, else -inf */
#define VAG_PRIOR_NONE 3        /* 0 inside the bounds: the caller adds its own ln prior for this parameter */
#define VAG_PRIOR_UNIFORM_RANGE 4 /* ABI v9: bilby Uniform(minimum = prior_a, maximum = prior_b) with its OWN support:
                                   * -ln(max - min) for min <= x <= max, else -inf (narrower or wider than the bounds) */

/* theta is [nb][ndim] (host); out is [nb] log-likelihoods (host).  Walkers whose
 * transformed parameters fail validation get -inf, like eval_one's except branch. */
int vag_loglike_batch(vag_ctx* ctx, const vag_fit_spec* spec, const double* theta, int nb, int ndim, double* out);

/* vag_loglike_batch(_dev) with VLBI centroid groups: after the flux and band passes, every group of sky (NULL or n_groups = 0: none)
 * runs as its own request and adds its chi^2 term (vag_centroid_obs).  Free parameters may also take the slots VAG_P_SKY_*.  A
 * walker whose F <= 0 or non-finite moments at a centroid epoch, or whose centroid pass fails (grid, ODE rows, SSC tables), scores
 * -inf.  With no centroid groups the result is bit for bit vag_loglike_batch's.  theta / out: host (vag_loglike_sky_batch) or device
 * (vag_loglike_sky_batch_dev) pointers.  Added after VAG_ABI_VERSION 13 (detect by symbol). */
int vag_loglike_sky_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const double* theta, int nb, int ndim,
                          double* out);
int vag_loglike_sky_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const double* d_theta, int nb,
                              int ndim, double* d_out);

/* One group of VLBI visibilities at one frequency (added after VAG_ABI_VERSION 13, detect by symbol): n_epochs strictly ascending
 * times, and for every epoch its own list of baselines with the measured complex visibility (ragged: first[]).  The group is its own
 * request (own grid from its own times).  The model visibility is
 *   V_mod(u, v) = exp(-2 pi i (u east0 + v north0)) V_sky(u, v; PA, n_az)
 * with V_sky exactly the Fourier sum of vag_sky_visibility_batch and PA / east0 / north0 the walker's sky placement (VAG_P_SKY_*,
 * shared with the centroid groups).  kind = VAG_VIS_COMPLEX adds sum_k weight_k |V_obs,k - V_mod,k|^2 / err_k^2 to the walker's
 * chi^2, kind = VAG_VIS_AMPLITUDE adds sum_k weight_k (re_k - |V_mod,k|)^2 / err_k^2 (east0 / north0 drop out).  Weights are used as
 * given.  Limits: at most VAG_VIS_MAX_GROUPS groups, VAG_VIS_MAX_EPOCHS epochs per group and VAG_VIS_MAX_PER_EPOCH visibilities per
 * epoch; more is refused with VAG_E_INVALID. */
#define VAG_VIS_COMPLEX 0
#define VAG_VIS_AMPLITUDE 1
#define VAG_VIS_MAX_GROUPS 64
#define VAG_VIS_MAX_EPOCHS 4096
#define VAG_VIS_MAX_PER_EPOCH VAG_SKY_MAX_BASELINES
typedef struct vag_visibility_obs {
    double nu;             /* [Hz] */
    int32_t n_epochs;      /* >= 1 */
    int32_t n_vis;         /* all epochs together, >= 1 */
    int32_t n_az;          /* azimuthal parts per circle of the model (vag_sky_visibility_batch); <= 0: 1024 */
    int32_t kind;          /* VAG_VIS_COMPLEX / VAG_VIS_AMPLITUDE */
    const double* t;       /* [n_epochs] strictly ascending [s] */
    const int32_t* first;  /* [n_epochs + 1]: epoch e owns the visibilities first[e] .. first[e + 1] - 1; first[0] = 0,
                              first[n_epochs] = n_vis, every epoch non-empty */
    const double* u;       /* [n_vis] east  [wavelengths] */
    const double* v;       /* [n_vis] north [wavelengths] */
    const double* re;      /* [n_vis] Re V_obs, or the amplitude (kind = AMPLITUDE); units of vag_flux_density_grid_batch */
    const double* im;      /* [n_vis] Im V_obs; ignored (may be NULL) for kind = AMPLITUDE */
    const double* err;     /* [n_vis] > 0: standard deviation of the real and of the imaginary part */
    const double* weight;  /* [n_vis] >= 0 */
} vag_visibility_obs;

typedef struct vag_vis_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_visibility_obs* groups; /* [n_groups] */
} vag_vis_fit_spec;

/* vag_loglike_sky_batch(_dev) with visibility groups: after the flux, band and centroid passes every group of vis runs as its own
 * pass and adds its chi^2 term (vag_visibility_obs), formed on the device; no visibility leaves it.  sky may be NULL (no centroid
 * groups, placement 0) or have n_groups = 0 and still supply pa_fixed / east0_fixed / north0_fixed.  Free parameters may take the
 * slots VAG_P_SKY_* whenever centroid or visibility groups are present.  A walker whose visibility pass fails (grid, ODE rows, SSC
 * tables) or whose V_mod is not finite at a datum scores -inf; a model with no flux at an epoch is valid (V_mod = 0).  With vis NULL
 * or n_groups = 0 the call is vag_loglike_sky_batch(_dev), bit for bit.  Results are bitwise reproducible and a walker's value does
 * not depend on the rest of the batch.  The group data stay resident on the device by content hash. */
int vag_loglike_vis_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const double* theta, int nb, int ndim, double* out);
int vag_loglike_vis_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const double* d_theta, int nb, int ndim, double* d_out);

/* One group of polarization measurements at one frequency (added after VAG_ABI_VERSION 13, detect by symbol): n ascending times
 * with a measurement, errors and a weight each.  The group is its own request (own grid from its own times).  The model I, Q, U at
 * (t_i, nu) are exactly those of vag_sky_polarization_batch for the walker's parameters, the walker's vag_pol_spec (VAG_P_POL_*, else
 * the fixed values of vag_pol_fit_spec), the walker's position angle (VAG_P_SKY_PA, shared with the centroid and visibility groups)
 * and the group's n_az.  kind = VAG_POL_QU: q, u are Q/I and U/I on the sky (IAU) and the group adds
 *   sum_i weight_i [((q_i - Q_sky/I) / err_q_i)^2 + ((u_i - U_sky/I) / err_u_i)^2]
 * to the walker's chi^2; kind = VAG_POL_DEGREE: q, err_q hold the degree Pi_i and its error, u and err_u are ignored (may be NULL),
 * and the group adds sum_i weight_i ((Pi_i - hypot(Q, U)/I) / err_q_i)^2 (the position angle drops out).  Weights are used as given.
 * Limits: at most VAG_POL_MAX_GROUPS groups of at most VAG_VIS_MAX_EPOCHS epochs; more is refused with VAG_E_INVALID.  Upper
 * limits on the degree (kind = VAG_POL_DEGREE) are supported through vag_loglike_lim_batch (vag_limit_fit_spec.pol_kind); upper
 * limits on q / u, on visibilities and on centroids, circular polarization and several frequencies in one group are not supported. */
#define VAG_POL_QU 0
#define VAG_POL_DEGREE 1
#define VAG_POL_MAX_GROUPS 64
typedef struct vag_polarization_obs {
    double nu;            /* [Hz] */
    int32_t n;            /* epochs, >= 1 */
    int32_t n_az;         /* azimuthal parts per circle of the model (vag_sky_polarization_batch); <= 0: 256 */
    int32_t kind;         /* VAG_POL_QU / VAG_POL_DEGREE */
    int32_t pad;
    const double* t;      /* [n] ascending, > 0 [s] */
    const double* q;      /* [n] Q/I on the sky, or the degree (kind = DEGREE) */
    const double* u;      /* [n] U/I on the sky; ignored for kind = DEGREE */
    const double* err_q;  /* [n] > 0 */
    const double* err_u;  /* [n] > 0; ignored for kind = DEGREE */
    const double* weight; /* [n] >= 0 */
} vag_polarization_obs;

/* The polarization groups of a likelihood call and the values of the VAG_P_POL_* parameters that are not free (index 0: forward
 * shock, 1: reverse shock): pi_max_fixed[e] < 0: (p + 1) / (p + 7/3) with the walker's own p of that shock; b_fixed[1] < 0: the
 * reverse shock follows the walker's forward b. */
typedef struct vag_pol_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_polarization_obs* groups; /* [n_groups] */
    double b_fixed[2];
    double pi_max_fixed[2];
} vag_pol_fit_spec;

/* vag_loglike_vis_batch(_dev) with polarization groups: after the flux, band, centroid and visibility passes every group of pol
 * runs as its own pass and adds its chi^2 term (vag_polarization_obs), formed on the device; no Stokes value leaves it.  sky may be
 * NULL (position angle 0) or have n_groups = 0 and still supply pa_fixed.  Free parameters may take the slot VAG_P_SKY_PA and the
 * slots VAG_P_POL_* whenever a polarization group is present.  A walker scores -inf (and counts in n_walkers_rejected) when its own
 * vag_pol_spec would be refused by vag_sky_polarization_batch (b not finite or < 0, pi_max NaN or > 1), when a pass of a group fails
 * (grid, ODE rows, SSC tables), or when I <= 0 or I, Q or U is not finite at an epoch of a group (q is undefined there: the
 * centroid groups' F <= 0 rule).  With pol NULL or n_groups = 0 the call is vag_loglike_vis_batch(_dev), bit for bit.  Results are
 * bitwise reproducible and a walker's value does not depend on the rest of the batch.  The group data stay resident on the device
 * by content hash. */
int vag_loglike_pol_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const double* theta, int nb, int ndim, double* out);
int vag_loglike_pol_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const double* d_theta, int nb, int ndim, double* d_out);

/* Upper limits (non-detections) in the likelihood (added after VAG_ABI_VERSION 13, detect by symbol).  A limit row has a limit value
 * L and a noise level sigma > 0, both in the units of the datum it replaces, and adds
 *   -2 weight ln Phi((L - M) / sigma)
 * to the walker's chi^2 (ln L gains weight ln Phi(z)); Phi is the standard normal CDF, the weight is used as given, and M is the model
 * value: for a point row the model flux density after the extinction factor exp(-A_V k_i), without the 1e-300 clamp of the detection
 * term (a model with no flux satisfies a limit); for a row of a band group the band-integrated model flux; for a row of a
 * polarization group of kind VAG_POL_DEGREE hypot(Q, U) / I.  "A 3 sigma upper limit of X" is L = X, sigma = X / 3: the noise is
 * additive, so the term is in linear flux, not in ln F like the detections.  ln Phi is evaluated in FP64 in a form that stays finite
 * and accurate far into the tail (a model 1e6 sigma above a limit scores a finite, very negative value).
 * vag_limit_rows is parallel to the n rows it annotates: the rows keep their place in the sorted rows of vag_fit_spec / vag_band_obs
 * and ride in the pass that is evaluated anyway; on a limit row ln_flux / ln_err are ignored (the host writes 0 and 1 there). */
#define VAG_OBS_DETECTION 0
#define VAG_OBS_UPPER_LIMIT 1
typedef struct vag_limit_rows {      /* parallel to the n rows it annotates; kind == NULL: no limit row */
    const int32_t* kind;             /* [n] VAG_OBS_* */
    const double* limit;             /* [n] L  (read on limit rows only) */
    const double* sigma;             /* [n] > 0 (read on limit rows only) */
} vag_limit_rows;
typedef struct vag_limit_fit_spec {
    vag_limit_rows point;            /* parallel to spec->t[n_data] */
    int32_t n_bands, pad;            /* 0 or spec->n_bands */
    const vag_limit_rows* bands;     /* [n_bands], parallel to spec->bands[g] */
    int32_t n_pol_groups, pad2;      /* 0 or pol->n_groups */
    const int32_t* const* pol_kind;  /* [n_pol_groups] each [n] or NULL; L = q[i], sigma = err_q[i] of the group */
} vag_limit_fit_spec;

/* vag_loglike_pol_batch(_dev) with upper limits: every row flagged VAG_OBS_UPPER_LIMIT adds the limit term above instead of its
 * detection term, in the same pass and at the same place of the sum.  Validity is unchanged: a NaN model value makes chi^2
 * non-finite and the walker scores -inf, a polarization limit keeps its group's I <= 0 rule, a failed pass scores -inf; all of them
 * count in n_walkers_rejected.  Refused with VAG_E_INVALID (the message names the row): a kind other than VAG_OBS_*, a limit that
 * is not finite or (fluxes) < 0, a sigma that is not finite and > 0, a polarization limit outside [0, 1], a limit row in a
 * VAG_POL_QU group, n_bands / n_pol_groups that are neither 0 nor their partner's count.  With lim NULL or no limit row anywhere
 * the call is vag_loglike_pol_batch(_dev), bit for bit; a block whose kind is NULL (or all VAG_OBS_DETECTION) takes the same code
 * as there.  Results are bitwise reproducible and a walker's value does not depend on the rest of the batch.  The limit arrays stay
 * resident on the device by content hash. */
int vag_loglike_lim_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const double* theta, int nb, int ndim, double* out);
int vag_loglike_lim_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const double* d_theta, int nb, int ndim,
                              double* d_out);

/* Systematic and calibration errors per data set (added after VAG_ABI_VERSION 13, detect by symbol).  Each detection row -- a point
 * row or a row of a band group -- belongs to a noise group g in 0 .. n_groups - 1 (n_groups <= VAG_NOISE_MAX_GROUPS) or to none (-1).
 * A group has a fractional systematic s_g >= 0 (a free parameter with the slot VAG_P_NOISE_SYS0 + g, else sys_fixed[g]) and a
 * calibration fraction c_g >= 0 (calib[g], fixed per fit).  With f_i the model flux after the extinction factor,
 * r_i = ln F_obs,i - ln max(f_i, 1e-300), sigma_i the row's ln_err and w_i its weight, the grouped detection rows of group g add
 *   v_i = sigma_i^2 + s_g^2,  p_i = w_i / v_i,
 *   A = sum p_i r_i^2,  B = sum p_i r_i,  P = sum p_i,  N = sum w_i log1p(s_g^2 / sigma_i^2),
 *   chi^2_g = A - c_g^2 B^2 / (1 + c_g^2 P) + N + log1p(c_g^2 P)
 * to the walker's chi^2 in place of sum w_i (r_i / sigma_i)^2.  With all weights 1 this is r^T C^-1 r + ln det C - ln det diag(sigma^2)
 * for C = diag(sigma^2 + s^2) + c^2 1 1^T: the Gaussian in ln F with a common scale factor of prior width c marginalised, normalised
 * so that s = c = 0 is the fixed-error term.  Ungrouped rows keep that term; a row that vag_limit_fit_spec flags as an upper limit
 * keeps its limit term whatever its group id and does not enter A, B, P, N.  s_g may span the point rows and any number of band
 * groups (its sums are separable); a group with c_g > 0 must lie in one pass: point rows only, or exactly one band group. */
typedef struct vag_noise_fit_spec {
    int32_t n_groups;                /* 0 .. VAG_NOISE_MAX_GROUPS */
    int32_t n_bands;                 /* spec->n_bands */
    const int32_t* point_group;      /* [spec->n_data] group id or -1; NULL: no point row is grouped */
    const int32_t* band_group;       /* [n_bands] the group id of every row of band group b, or -1 */
    double sys_fixed[VAG_NOISE_MAX_GROUPS]; /* s_g of a group without a free parameter (0 when not given) */
    double calib[VAG_NOISE_MAX_GROUPS];     /* c_g */
} vag_noise_fit_spec;

/* vag_loglike_lim_batch(_dev) with noise groups.  With noise NULL or no grouped row it is exactly that call (lim may be NULL as
 * there); a pass without grouped rows launches what it launches there.  Validity, the evaluation order and the rejection counts are
 * unchanged.  Refused with VAG_E_INVALID: n_groups outside 0 .. VAG_NOISE_MAX_GROUPS, a group id outside [-1, n_groups), a sys_fixed
 * or calib that is negative or not finite, n_bands other than the fit spec's, a group with calib > 0 in more than one pass, and a
 * parameter slot VAG_P_NOISE_SYS0 + g without group g ("bad parameter slot").  Results are bitwise reproducible and a walker's value
 * does not depend on the rest of the batch.  The group ids stay resident on the device by content hash. */
int vag_loglike_noise_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                            const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                            const double* theta, int nb, int ndim, double* out);
int vag_loglike_noise_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                const double* d_theta, int nb, int ndim, double* d_out);

/* Photon counts with a Poisson likelihood (added after VAG_ABI_VERSION 13, detect by symbol).  A counts group is one band
 * (nu_min, nu_max, num_points Boole nodes, as vag_band_obs) with n rows; row i holds the observed counts N_i (a non-negative integer
 * carried as a double, at most 2^53), a background expectation B_i >= 0 [counts], a scale a_i > 0 [counts per erg cm^-2 s^-1 per
 * sample], a weight w_i >= 0 and m >= 1 indices into the group's sample times.  With F(t) the walker's band-integrated flux
 *   mu_i = B_i + a_i sum_{k = 0 .. m-1} F(t_sample[sample_idx[i m + k]])   (summed in k order),
 *   ln L += sum_i w_i [N_i ln mu_i - mu_i - ln N_i!],
 * formed as chi^2 += 2 sum_i w_i D_i - 2 sum_i w_i S_i with the deviance D_i = mu_i - N_i - N_i ln(mu_i / N_i) >= 0 (mu_i for
 * N_i = 0; vag::poisson_deviance, on the device) and the constant S_i = N_i ln N_i - N_i - ln N_i! (0 for N_i = 0; once per spec, on
 * the host).  mu_i = 0 with N_i > 0 scores -inf for the walker, with N_i = 0 it adds 0; a NaN model value scores -inf; a row with
 * w_i = 0 adds nothing whatever its model value.  Each group is its own pass: one band request on t_sample (its own grid from its own
 * times, as a band group), then vag_fit_back_counts_kernel. */
typedef struct vag_counts_obs {
    double nu_min, nu_max;      /* [Hz] */
    int32_t num_points;         /* Boole nodes across the band */
    int32_t n;                  /* rows */
    int32_t m;                  /* samples per row */
    int32_t n_samples;          /* distinct sample times */
    const double* t_sample;     /* [n_samples] strictly ascending, > 0 [s] */
    const int32_t* sample_idx;  /* [n * m] in [0, n_samples) */
    const double* counts;       /* [n] N_i */
    const double* background;   /* [n] B_i */
    const double* scale;        /* [n] a_i */
    const double* weight;       /* [n] w_i */
} vag_counts_obs;

typedef struct vag_counts_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_counts_obs* groups;  /* [n_groups] */
} vag_counts_fit_spec;

/* vag_loglike_noise_batch(_dev) with counts groups, which are passes of their own after the polarization groups.  With counts NULL
 * or n_groups == 0 it is exactly that call (the other specs may be NULL as there); the fit spec may then hold no other data.  A walker
 * a counts pass rejects (grid capacity, ODE rows, SSC tables) scores -inf and is counted like one a band group rejects.  Refused
 * with VAG_E_INVALID before the device is touched, the message naming group and row: counts that are not finite, negative, not an
 * integer or above 2^53; a background that is negative or not finite; a scale that is not finite and > 0; a weight that is negative or
 * not finite; n < 1, m < 1 or n_samples < 1; an index outside [0, n_samples); t_sample that is not finite, <= 0 or not strictly
 * ascending; a band or num_points that vag_band_obs would refuse; a null array.  Results are bitwise reproducible and do not depend
 * on the evaluation order.  A walker's counts term does not depend on the rest of the batch either, with two limits: every model of
 * the batches compared has at most 512 time nodes in its lattice (longer ones are summed in pieces), and for fits with SSC the choice
 * between the fused and the two-pass flux launch, which follows the batch's longest lattice, has not been shown to keep the bits.
 * (The other passes of the call keep their own behaviour: a band group's flux follows the batch in its last bits.)  The group arrays
 * stay resident on the device by content hash. */
int vag_loglike_counts_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                             const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                             const vag_counts_fit_spec* counts, const double* theta, int nb, int ndim, double* out);
int vag_loglike_counts_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                 const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                 const vag_counts_fit_spec* counts, const double* d_theta, int nb, int ndim, double* d_out);

/* Spectral indices (added after VAG_ABI_VERSION 13, detect by symbol).  A spectral-index group is k frequencies
 * nu_0 < .. < nu_{k-1} (2 <= k <= VAG_INDEX_MAX_NODES), k coefficients c_j (c_0 is carried but never read), a scalar ext_slope, and
 * n >= 1 rows (t_i, s_i, sigma_i, w_i); times are ascending, equal times are allowed.  With F the walker's flux density (the sum of
 * every enabled component, as for point rows) and A_V the walker's extinction (free or vag_fit_spec::a_v_fixed):
 *   S_i    = sum_{j = 1 .. k-1} c_j ln(F(t_i, nu_j) / F(t_i, nu_0)) - A_V ext_slope   (summed in j order; vag::log_slope),
 *   chi^2 += sum_i w_i ((S_i - s_i) / sigma_i)^2.
 * The pivot form is part of the definition: the sum is not sum_j c_j ln F_j (vag_index.h says why).  A row with w_i = 0 adds nothing
 * whatever its model values; a row with w_i > 0 at which some F(t_i, nu_j) is <= 0 or not finite makes the walker score -inf (the
 * slope is undefined; counted in n_walkers_rejected) -- the rule of the centroid and polarization groups, not the 1e-300 clamp of
 * the point rows.  Each group is its own pass: the n k points (t_i, nu_j), i outer, as one series request (the path of the point
 * rows, its own grid from its own times), then vag_fit_back_index_kernel. */
#define VAG_INDEX_MAX_NODES 8
typedef struct vag_index_obs {
    int32_t n;             /* rows */
    int32_t k;             /* frequencies */
    const double* nu;      /* [k] strictly ascending, > 0 [Hz] */
    const double* coef;    /* [k] c_j */
    double ext_slope;      /* sum_{j >= 1} c_j (kappa_j - kappa_0), kappa = 0.4 ln10 k(lambda_rest); 0 without an extinction law */
    const double* t;       /* [n] ascending, > 0 [s] */
    const double* value;   /* [n] s_i: the observed slope d ln F / d ln nu */
    const double* err;     /* [n] sigma_i > 0 */
    const double* weight;  /* [n] w_i >= 0 */
} vag_index_obs;

typedef struct vag_index_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_index_obs* groups;  /* [n_groups] */
} vag_index_fit_spec;

/* vag_loglike_counts_batch(_dev) with spectral-index groups, which are passes of their own after the counts groups.  With index NULL
 * or n_groups == 0 it is exactly that call (the other specs may be NULL as there); the fit spec may then hold no other data.  A
 * walker an index pass rejects (grid capacity, ODE rows, SSC tables) scores -inf and is counted like one any other pass rejects.
 * Refused with VAG_E_INVALID before the device is touched, the message naming group and row: k outside 2..VAG_INDEX_MAX_NODES; a
 * frequency that is not finite, not positive or not strictly ascending; a coefficient or ext_slope that is not finite; a time that
 * is not finite, <= 0 or descending; a value that is not finite; an err that is not finite and > 0; a weight that is negative or
 * not finite; a null array; n < 1.  Results are bitwise reproducible.  The group arrays stay resident on the device by content
 * hash. */
int vag_loglike_index_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                            const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                            const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const double* theta, int nb, int ndim,
                            double* out);
int vag_loglike_index_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                                const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                                const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const double* d_theta, int nb,
                                int ndim, double* d_out);

/* Count spectra through an instrument response (added after VAG_ABI_VERSION 13, detect by symbol).  A fold group holds J energy bins
 * [E_lo_j, E_hi_j] [keV, observer frame; 0 < E_lo_j < E_hi_j, ascending, non-overlapping, gaps allowed], C channels, a response
 * R[c][j] >= 0 [cm^2: counts in channel c per photon cm^-2 arriving in bin j; the caller rebins the instrument's matrix to these bins
 * and folds in any fixed Galactic absorption], n spectra (rows) with t_start_i, exposure_i, observed counts N[i][c], a background
 * expectation B[i][c] >= 0 and weights w[i][c] >= 0 (w = 0 ignores a channel), m samples per window on the merged, strictly ascending
 * t_sample list of the counts groups, and optionally a cross-section sigma_j >= 0 [cm^2 per H atom] at each bin, as the caller's
 * table gives it for the absorber's redshift (the engine does not shift it).  With h Planck's constant [erg s]:
 *   nodes        nu_j = sqrt(E_lo_j E_hi_j) keV / h;
 *   host matrix  A[j][c] = R[c][j] ln(E_hi_j / E_lo_j) / h   [counts s^-1 per erg cm^-2 s^-1 Hz^-1]: the midpoint rule in ln E of
 *                int_bin N_E dE = int (F_nu / h) d ln E; for F_nu ~ nu^-beta the folded value over the exact one is x / sinh x,
 *                x = beta ln(E_hi / E_lo) / 2;
 *   per walker   T_j = exp(-N_H sigma_j), or 1 without sigma (N_H: the free parameter with the slot VAG_P_N_H, else n_h_fixed);
 *   G[i][j]  = T_j ((exposure_i / m) sum_s F_nu(t_sample[sample_idx[i m + s]], nu_j))   (summed in s order; F_nu the total of every
 *              enabled component, as for point rows);
 *   mu[i][c] = B[i][c] + sum_j A[j][c] G[i][j]   (summed in ascending j from 0, one fma per term, B added last; vag::fold_mu);
 *   ln L += sum_{i,c} w [N ln mu - mu - ln N!],
 * formed as chi^2 += 2 sum w D(N, mu) + const2 with vag::poisson_deviance and the host-side constant exactly as for counts groups.
 * mu = 0 with N > 0 and w > 0 scores -inf; mu = 0 with N = 0 adds 0; a NaN model value scores -inf; w = 0 adds nothing whatever
 * the model value; a walker the pass rejects (grid capacity, ODE rows, SSC tables) scores -inf and is counted in n_walkers_rejected.
 * Each group is its own pass after the index groups: the n_samples J points (t, nu), t outer and nu inner, as one series request (the
 * path of the point rows; it goes through in chunks above 512 points), then vag_fit_back_fold_kernel.  The struct carries nu and A,
 * not the bins and R. */
#define VAG_FOLD_MAX_BINS 64
#define VAG_FOLD_MAX_CHANNELS 256
typedef struct vag_fold_obs {
    int32_t J;                     /* energy bins, 1 .. VAG_FOLD_MAX_BINS */
    int32_t C;                     /* channels, 1 .. VAG_FOLD_MAX_CHANNELS */
    int32_t n;                     /* spectra (rows) */
    int32_t m;                     /* samples per row */
    int32_t n_samples;             /* distinct sample times */
    int32_t pad;
    const double* nu;              /* [J] strictly ascending, > 0 [Hz] */
    const double* A;               /* [J * C] A[j][c] >= 0 */
    const double* sigma;           /* [J] sigma_j >= 0 [cm^2], or NULL: no absorber */
    const double* t_sample;        /* [n_samples] strictly ascending, > 0 [s] */
    const int32_t* sample_idx;     /* [n * m] in [0, n_samples) */
    const double* exposure_over_m; /* [n] exposure_i / m > 0 [s] */
    const double* counts;          /* [n * C] N[i][c]: non-negative integers carried as doubles, at most 2^53 */
    const double* background;      /* [n * C] B[i][c] >= 0 */
    const double* weight;          /* [n * C] w[i][c] >= 0 */
} vag_fold_obs;

typedef struct vag_fold_fit_spec {
    int32_t n_groups;
    int32_t pad;
    const vag_fold_obs* groups;  /* [n_groups] */
    double n_h_fixed;            /* N_H [cm^-2] when it is not a free parameter; one N_H serves every group that carries a sigma */
} vag_fold_fit_spec;

/* vag_loglike_index_batch(_dev) with fold groups, which are passes of their own after the index groups.  With fold NULL or
 * n_groups == 0 it is exactly that call (the other specs may be NULL as there); the fit spec may then hold no other data.  Refused
 * with VAG_E_INVALID before the device is touched, the message naming group, row and channel: J, C outside their caps, n < 1, m < 1,
 * n_samples < 1; a null array; an entry of A, sigma, background or weight that is negative or not finite; counts that are not
 * non-negative integers <= 2^53; nu that is not finite, > 0 and strictly ascending; t_sample that is not finite, > 0 and strictly
 * ascending; an index outside [0, n_samples); an exposure_over_m that is not finite and > 0; an n_h_fixed that is negative or not
 * finite; a free parameter with the slot VAG_P_N_H when no group has sigma ("bad parameter slot").  Results are bitwise
 * reproducible.  The group arrays stay resident on the device by content hash. */
int vag_loglike_fold_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                           const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                           const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                           const double* theta, int nb, int ndim, double* out);
int vag_loglike_fold_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                               const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                               const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                               const double* d_theta, int nb, int ndim, double* d_out);

/* Additive templates in the flux passes (added after VAG_ABI_VERSION 13, detect by symbol): a host galaxy's constant flux, a supernova
 * or kilonova bump -- a fixed shape per data set whose amplitude is a fit parameter.  A fit has up to VAG_TMPL_MAX templates.
 * Template c has an amplitude a_c >= 0 (the free parameter with the slot VAG_P_TMPL_AMP0 + c, else amp_fixed[c]), a flag
 * extinguished[c], and a value T_c,i >= 0, finite, for every row i of every flux pass (the point rows, a band group); T_c,i = 0:
 * the template does not touch the row.  With F_i the walker's model flux at the row (band-integrated for a band row) the row's
 * model value becomes
 *   e_i = sum_c a_c T_c,i over the templates with extinguished = 0,
 *   x_i = sum_c a_c T_c,i over the templates with extinguished = 1,
 *   f_i = (F_i + x_i) exp(-A_V k_i) + e_i
 * (both sums from 0 in ascending c, one fma per term; the extinction factor exactly where it applies today: a pass without an
 * extinction kernel has factor 1).  f_i replaces the model value in every term a flux pass forms: the detection term with its 1e-300
 * clamp and NaN rule, the limit term (no clamp), and r_i of the noise-group sums.  Nothing else reads templates: counts, index, fold,
 * centroid, visibility and polarization groups do not.  Units are the row's own: a point-row template is in the unit of the flux
 * density at T = 1, a band-row template in erg cm^-2 s^-1.  A walker whose free amplitude is not finite or is negative scores -inf
 * and is counted in vag_plan.n_walkers_rejected. */
typedef struct vag_template_fit_spec {
    int32_t n_templates;               /* 0 .. VAG_TMPL_MAX */
    int32_t n_bands;                   /* 0 or spec->n_bands */
    const double* point;               /* [n_templates][spec->n_data] row-major, or NULL: no template touches a point row */
    const double* const* bands;        /* [n_bands]: each [n_templates][n of that band group], or NULL */
    double  amp_fixed[VAG_TMPL_MAX];   /* a_c of a template without a free parameter */
    int32_t extinguished[VAG_TMPL_MAX]; /* 1: the template is behind the host's dust (x_i), 0: it is not (e_i) */
} vag_template_fit_spec;

/* vag_loglike_fold_batch(_dev) with templates.  With tmpl NULL or no touched row (every T = 0) it is exactly that call, bit for
 * bit; a pass no template touches launches what it launches there.  Refused with VAG_E_INVALID before the device is touched, the
 * message naming template and row: n_templates outside 0 .. VAG_TMPL_MAX; n_bands neither 0 nor the fit spec's; an entry of T that
 * is negative or not finite; an amp_fixed that is negative or not finite; an extinguished other than 0 or 1; a parameter slot
 * VAG_P_TMPL_AMP0 + c with c >= n_templates ("bad parameter slot").  Results are bitwise reproducible and a walker's value does not
 * depend on the rest of the batch or on its evaluation slot.  The template values stay resident on the device by content hash. */
int vag_loglike_tmpl_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                           const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                           const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                           const vag_template_fit_spec* tmpl, const double* theta, int nb, int ndim, double* out);
int vag_loglike_tmpl_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                               const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                               const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                               const vag_template_fit_spec* tmpl, const double* d_theta, int nb, int ndim, double* d_out);

/* Correlated errors (added after VAG_ABI_VERSION 13, detect by symbol): radio light curves with interstellar scintillation,
 * photometry that shares a zero point or a host subtraction, unfolded spectra with correlated bins.  A correlated group is n rows
 * (t_i, nu_i), 1 <= n <= VAG_COV_MAX_ROWS; a fit holds at most VAG_COV_MAX_GROUPS groups.  Each group has rows with times ascending
 * (equal times allowed), observed log fluxes ln_flux[i], an optional extinction kernel ext[i] = 0.4 ln10 k(lambda_rest) as on the
 * point rows, a scalar weight w >= 0, and a whitener W: lower triangular with positive diagonal, W C_ln W^T = I, C_ln the covariance
 * of the ln F_obs.  With F the walker's flux density at the rows, the sum of every enabled component as for point rows,
 *   f_i = F_i exp(-A_V ext_i)               (the factor only when ext is given and A_V != 0, as vag_fit_back_kernel)
 *   r_i = ln_flux_i - ln max(f_i, 1e-300)   (a NaN f_i stays NaN: the walker scores -inf)
 *   y_i = sum_{j=0..i} W_ij r_j             (from 0, ascending j, one fma per term)
 *   chi^2 += w sum_i y_i^2                  (lane-strided sums closed by wave_sum, the fixed order of the other back kernels)
 * This is w r^T C_ln^-1 r.  The walker-independent ln det C_ln is not added, just as the plain chi^2 carries no sum ln sigma^2.  With
 * C_ln = diag(sigma_ln^2) the term is the point rows' sum ((ln F_obs - ln f) / sigma_ln)^2; with C_ln = diag(sigma_ln^2) + c^2 1 1^T
 * it is the calibration group's r^T C^-1 r.  Each group is a pass of its own, after the fold groups: one series request at its n
 * points, then vag_fit_back_cov_kernel; a group with w = 0 still makes its request (the walker's validity is that of the pass) and
 * adds 0.  A fit may hold nothing but correlated groups.  Out of scope: a free jitter or systematic on a correlated group, upper
 * limits and templates inside one, correlations across groups, band-integrated rows with a covariance, n > VAG_COV_MAX_ROWS, and
 * sharded calls. */
#define VAG_COV_MAX_ROWS 256
#define VAG_COV_MAX_GROUPS 8
typedef struct vag_cov_obs {
    int32_t n;                /* rows, 1 .. VAG_COV_MAX_ROWS */
    const double* t;          /* [n] s, ascending */
    const double* nu;         /* [n] Hz */
    const double* ln_flux;    /* [n] ln F_obs */
    const double* ext;        /* [n] 0.4 ln10 k(lambda_rest), or NULL */
    const double* whitener;   /* [n][n] row-major; the entries j <= i are read */
    double weight;            /* w >= 0 */
} vag_cov_obs;
typedef struct vag_cov_fit_spec {
    int32_t n_groups;         /* 0 .. VAG_COV_MAX_GROUPS */
    const vag_cov_obs* groups;
} vag_cov_fit_spec;

/* vag_loglike_tmpl_batch(_dev) with correlated groups.  With cov NULL or n_groups = 0 it is exactly that call, bit for bit: a fit
 * without correlated groups launches what it launches there.  Refused with VAG_E_INVALID before the device is touched, the message
 * naming group and row: n outside 1 .. VAG_COV_MAX_ROWS or n_groups outside 0 .. VAG_COV_MAX_GROUPS; a null array; a t or nu that is
 * not finite or not positive, or descending t; a ln_flux or ext that is not finite; a whitener entry with j <= i that is not finite,
 * or a diagonal entry <= 0; a weight that is negative or not finite.  A walker the pass rejects (grid capacity, ODE rows, SSC tables)
 * scores -inf and is counted in vag_plan.n_walkers_rejected.  Results are bitwise reproducible and a walker's term does not depend on
 * the rest of the batch or on its evaluation slot, under the conditions the index groups state.  The groups stay resident on the
 * device by content hash, W stored transposed. */
int vag_loglike_cov_batch(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                          const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                          const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                          const vag_template_fit_spec* tmpl, const vag_cov_fit_spec* cov, const double* theta, int nb, int ndim,
                          double* out);
int vag_loglike_cov_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const vag_sky_fit_spec* sky, const vag_vis_fit_spec* vis,
                              const vag_pol_fit_spec* pol, const vag_limit_fit_spec* lim, const vag_noise_fit_spec* noise,
                              const vag_counts_fit_spec* counts, const vag_index_fit_spec* index, const vag_fold_fit_spec* fold,
                              const vag_template_fit_spec* tmpl, const vag_cov_fit_spec* cov, const double* d_theta, int nb, int ndim,
                              double* d_out);

/* The ensemble sampler on the device (added after VAG_ABI_VERSION 13, detect by symbol): the Goodman & Weare stretch move in its
 * parallel form with fixed halves (Foreman-Mackey et al. 2013, section 3).  n_walkers is even and >= 2 ndim; half 0 is walkers
 * [0, n_walkers / 2), half 1 the rest; a step updates half 0 against half 1, then half 1 against the updated half 0; there is no
 * permutation.  The draws are Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85) with key
 * (seed & 0xffffffff, seed >> 32) and counter (w, step & 0xffffffff, step >> 32, stream): w the walker's index in the whole
 * ensemble, step the absolute step number, stream 0 the proposal and 1 the acceptance.  A uniform of two output words is
 * u(hi, lo) = ((hi >> 5) 2^26 + (lo >> 6)) 2^-53.  With x0..x3 of stream 0: u_z = u(x0, x1), the partner is walker
 * (uint64(x2) half) >> 32 of the other half, t = fma(a - 1, u_z, 1), z = t t / a (the largest double below a where that quotient reaches a), prop[d] = fma(z, pos[w][d] - pos[partner][d],
 * pos[partner][d]).  With y0, y1 of stream 1: u_a = u(y0, y1); a proposal whose ln p is not finite is rejected, any other is accepted
 * iff log(u_a) < (ndim - 1) log(z) + (lp_new - lp[w]).  A chain is therefore a function of (seed, step, walker) and of ln p alone. */
/* Outlier groups (added after VAG_ABI_VERSION 13, detect by symbol): the mixture ("good / bad data") likelihood of Hogg, Bovy & Lang
 * (2010, section 3) per data set.  An outlier group is a noise group g of vag_noise_fit_spec whose bit is set in `mask`.  It has three
 * more parameters, each a free parameter or fixed: the outlier fraction P_g in [0, 1) (slot VAG_P_ROBUST_FRAC0 + g, else
 * frac_fixed[g]), the extra scatter of outliers in ln F b_g >= 0 (VAG_P_ROBUST_SCALE0 + g, else scale_fixed[g]) and their mean offset
 * in ln F mu_g, finite (VAG_P_ROBUST_SHIFT0 + g, else shift_fixed[g]).  With f_i the model value exactly as the template kernel forms
 * it (templates, then extinction), r_i = ln F_obs,i - ln max(f_i, 1e-300) (a NaN stays NaN), sigma_i the row's ln_err, w_i its weight
 * and s_g the group's systematic, every detection row of the group adds
 *   v_in = sigma_i^2 + s_g^2,  v_out = v_in + b_g^2,
 *   g_i = log1p(-P_g) - r_i^2 / (2 v_in)           - log1p(s_g^2 / sigma_i^2) / 2
 *   o_i = ln P_g      - (r_i - mu_g)^2 / (2 v_out) - log1p((s_g^2 + b_g^2) / sigma_i^2) / 2
 *   l_i = max(g_i, o_i) + log1p(exp(-|g_i - o_i|)),      chi^2 += -2 sum_i w_i l_i
 * (a lane-strided sum closed by wave_sum, as the other back kernels) in place of the noise group's A + N.  ln 0 = -inf is used as it
 * stands: P_g = 0 gives l_i = g_i, the noise group's term of the row.  exp(l_i) / (sqrt(2 pi) sigma_i) integrates to 1 over r_i, as the
 * noise group's term does, so P, b and s can all be sampled; the row's outlier probability is exp(o_i - l_i).  Upper-limit rows of a
 * robust group keep their limit term; ungrouped rows and the groups without the bit keep their terms statement for statement.  A
 * robust group may span the point rows and any number of band groups (the sum is separable) and may not have calib > 0: the rank-one
 * marginalisation does not commute with the mixture.  A walker whose free P_g is not finite or lies outside [0, 1), whose free b_g is
 * not finite or is negative, or whose free mu_g is not finite scores -inf and is counted in vag_plan.n_walkers_rejected.  Out of
 * scope: outliers on counts, index, fold, correlated, centroid, visibility and polarization groups, more than two components, per-row
 * prior probabilities, and sharded calls. */
typedef struct vag_robust_fit_spec {
    int32_t n_groups;                         /* the noise spec's n_groups */
    uint32_t mask;                            /* bit g: group g is robust */
    double frac_fixed[VAG_NOISE_MAX_GROUPS];  /* P_g of a group without a free parameter, in [0, 1) (0 when not given) */
    double scale_fixed[VAG_NOISE_MAX_GROUPS]; /* b_g, >= 0 */
    double shift_fixed[VAG_NOISE_MAX_GROUPS]; /* mu_g, finite */
} vag_robust_fit_spec;

/* The spec blocks of a likelihood call; a null pointer: the block is absent.  `robust` is the twelfth member, added with the outlier
 * groups: a caller compiled against the eleven-member struct must be rebuilt (the entry points read the member). */
typedef struct vag_loglike_request {
    const vag_fit_spec* spec;
    const vag_sky_fit_spec* sky;
    const vag_vis_fit_spec* vis;
    const vag_pol_fit_spec* pol;
    const vag_limit_fit_spec* lim;
    const vag_noise_fit_spec* noise;
    const vag_counts_fit_spec* counts;
    const vag_index_fit_spec* index;
    const vag_fold_fit_spec* fold;
    const vag_template_fit_spec* tmpl;
    const vag_cov_fit_spec* cov;
    const vag_robust_fit_spec* robust;
} vag_loglike_request;

/* vag_loglike_cov_batch(_dev) in the request form, with outlier groups.  With request->robust NULL, or when no detection row lies in
 * a robust group, the call is vag_loglike_cov_batch(_dev) of the request's other blocks, bit for bit: a pass without a detection row
 * of a robust group launches what it launches there; a pass with one launches vag_fit_back_robust_kernel.  vag_stretch_run_dev,
 * vag_move_run_dev, vag_tempered_run_dev, vag_nested_run_dev and vag_loglike_split_dev take the block through their request.  Refused
 * with VAG_E_INVALID before the device is touched, the message naming the group: a robust block without a noise block; n_groups other
 * than the noise spec's; a mask bit at or above n_groups; a robust group with calib > 0; a frac_fixed that is not finite or outside
 * [0, 1); a scale_fixed that is not finite or negative; a shift_fixed that is not finite; and a parameter slot VAG_P_ROBUST_* + g for
 * a group that is not robust ("bad parameter slot").  Results are bitwise reproducible, and a walker's value does not depend on the
 * rest of the batch or on its evaluation slot.  The 24 fixed values stay resident on the device by content hash. */
int vag_loglike_robust_batch(vag_ctx* ctx, const vag_loglike_request* request, const double* theta, int nb, int ndim, double* out);
int vag_loglike_robust_batch_dev(vag_ctx* ctx, const vag_loglike_request* request, const double* d_theta, int nb, int ndim,
                                 double* d_out);
typedef struct vag_stretch_spec {
    uint64_t seed;
    double a;           /* the stretch scale, finite and > 1 (2 is customary) */
    int32_t n_walkers;  /* even, >= 2 ndim */
    int32_t ndim;       /* 1 .. 16 */
    int32_t thin;       /* >= 1: step s is stored when (s + 1) % thin == 0 */
} vag_stretch_spec;

/* The two halves of a half-step as building blocks (no model): a caller with an evaluator of its own -- a sharded one -- puts its
 * call between them.  half is 0 or 1; d_pos[n_walkers][ndim], d_prop[n_walkers / 2][ndim] the proposals of the half's walkers in
 * their order, d_lp_new[n_walkers / 2] their ln p, d_lp[n_walkers] ln p of d_pos, d_accepted[n_walkers] counts.  Stream-ordered on
 * the context's stream, no host synchronisation.  Refused with VAG_E_INVALID (the context stays usable): a null context, spec or
 * buffer; n_walkers odd or < 2 ndim; ndim outside 1 .. 16; a not finite or <= 1; thin < 1; half not 0 or 1. */
int vag_stretch_propose_dev(vag_ctx* ctx, const vag_stretch_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop);
int vag_stretch_accept_dev(vag_ctx* ctx, const vag_stretch_spec* sp, uint64_t step, int half, const double* d_prop,
                           const double* d_lp_new, double* d_pos, double* d_lp, int64_t* d_accepted);

/* Steps step0 .. step0 + n_steps - 1 of the move on the likelihood of `request` (ln L + ln prior with the bounds mask under
 * spec->use_priors): per step and half, propose, the likelihood call of the n_walkers / 2 proposals, accept.  On entry d_lp holds
 * ln p of d_pos.  The blocks are scanned and uploaded once per call; between the steps there is no copy and no stream synchronisation
 * (a likelihood call itself waits for its device plan, as vag_loglike_batch_dev does).  A stored step writes its row
 * [n_walkers][ndim] of d_chain and [n_walkers] of d_logp; rows are consecutive from the pointers given, which the caller sizes and
 * moves between calls; both null: nothing is stored.  n_steps = 0 does nothing and returns VAG_OK.  Refusals as above, and:
 * a null request or request->spec, ndim different from request->spec->ndim, n_steps < 0, one of d_chain / d_logp null alone, and
 * whatever the likelihood call refuses. */
int vag_stretch_run_dev(vag_ctx* ctx, const vag_loglike_request* request, const vag_stretch_spec* sp, uint64_t step0, int n_steps,
                        double* d_pos, double* d_lp, int64_t* d_accepted, double* d_chain, double* d_logp);

/* The move mix of the device sampler (added after VAG_ABI_VERSION 13, detect by symbol): the stretch move, the differential-evolution
 * move (ter Braak 2006, with the scale jitter of Nelson et al. 2013 that emcee 3 uses) and the snooker move (ter Braak & Vrugt 2008),
 * chosen per step by weight.  The reference's emcee configuration is DE at 0.8 and snooker at 0.2.  The framing is that of
 * vag_stretch_*: nh = n_walkers / 2, half h is updated against the other half, which does not move during that half-step; the draws
 * are Philox4x32-10 with the key and the counter (w, step & 0xffffffff, step >> 32, stream) described above.  Streams 0 (proposal),
 * 1 (acceptance) and 2 (exchange, tempering) keep their meaning; stream 3 is the move choice and stream 4 a second block of proposal
 * words.  x0..x3 are the words of stream 0 at walker w, v0..v3 those of stream 4, u(hi, lo) the uniform above.
 * The choice: one per step, shared by both halves.  With u_c = u of the first two words of counter (0, step lo, step hi, 3) and the
 * weights (w_s, w_de, w_sn) = weights[VAG_MOVE_*] (non-negative, finite, sum > 0; only their ratios matter): t = u_c ((w_s + w_de) +
 * w_sn); the stretch move if t < w_s, else DE if t < w_s + w_de, else snooker.  The host evaluates this and launches the kernel of
 * the kind; a kind of weight 0 is never chosen.
 * The stretch kind: vag_stretch_propose_dev's proposal, bit for bit, and factor = (ndim - 1) log(z).
 * The DE kind (nh >= 2): walker w draws a != b of the other half, a = (uint64(x2) nh) >> 32, b = (a + 1 + ((uint64(x3) (nh - 1))
 * >> 32)) mod nh, and a standard normal n = sqrt(-2 log(1 - u(x0, x1))) cos(2 pi u(v0, v1)) (2 pi the double 6.283185307179586),
 * which is quantised to a multiple of 2^-20, n_q = rint(n 2^20) 2^-20 (this changes gamma by 1e-11 relative: of no statistical
 * consequence; it makes n_q independent of the last bits of log and cos unless n 2^20 lies within their rounding, about 1e-9, of a
 * half-integer).  gamma = gamma0 fma(sigma, n_q, 1), gamma0 = 0 standing for 2.38 / sqrt(2 ndim); prop[d] = fma(gamma, pos[a][d] -
 * pos[b][d], pos[w][d]); factor = 0.
 * The snooker kind (nh >= 3): walker w draws three distinct walkers z, z1, z2 of the other half: z and z1 as a and b above, z2 =
 * (uint64(v2) (nh - 2)) >> 32 stepped over the two taken indices in ascending order (+1 if >= the smaller, then +1 if >= the larger).
 * With delta = pos[w] - pos[z], r2 = delta . delta and proj = delta . (pos[z1] - pos[z2]) (both summed from 0 in ascending d, one fma
 * per term): c = gamma_snooker (proj / r2), prop[d] = fma(c, delta[d], pos[w][d]), and factor = ((ndim - 1) / 2) log(|prop - pos[z]|^2
 * / r2), the squared norm summed the same way.  This projects z1 - z2 on the UNIT vector along delta, as the paper does (emcee's
 * DESnookerMove divides delta by sqrt(|delta|) instead, which is not a unit vector: its step carries a factor |delta|).  A walker with r2 = 0, or
 * whose factor is not finite, proposes its own position with factor = -inf and is rejected.
 * The acceptance, for every kind: a proposal whose ln p is not finite is rejected; any other is accepted iff
 * log(u_a) < factor + (lp_new - lp[w]), u_a = u(y0, y1) of stream 1 exactly as in vag_stretch_accept_dev. */
#define VAG_MOVE_STRETCH 0
#define VAG_MOVE_DE 1
#define VAG_MOVE_SNOOKER 2
typedef struct vag_move_spec {
    uint64_t seed;
    double a;              /* the stretch scale, finite and > 1 (checked whatever the weights) */
    double gamma0;         /* the DE scale, finite and >= 0; 0: the default 2.38 / sqrt(2 ndim) */
    double sigma;          /* the relative jitter of the DE scale, finite (1e-5 is customary) */
    double gamma_snooker;  /* the snooker scale, finite (1.7 is customary) */
    double weights[3];     /* by VAG_MOVE_*: finite, >= 0, not all zero */
    int32_t n_walkers;     /* even, >= 2 ndim; >= 4 with weights[VAG_MOVE_DE] > 0, >= 6 with weights[VAG_MOVE_SNOOKER] > 0 */
    int32_t ndim;          /* 1 .. 16 */
    int32_t thin;          /* >= 1: step s is stored when (s + 1) % thin == 0 */
} vag_move_spec;

/* The building blocks, as vag_stretch_propose_dev / vag_stretch_accept_dev with d_factor[n_walkers / 2] between them: propose writes
 * the ln of the Hastings factor of each proposal, accept reads it.  Stream-ordered on the context's stream, no host synchronisation.
 * Refused with VAG_E_INVALID (the context stays usable): whatever the stretch entries refuse; a weight that is negative or not
 * finite, or all three zero; weights[VAG_MOVE_DE] > 0 with n_walkers / 2 < 2; weights[VAG_MOVE_SNOOKER] > 0 with n_walkers / 2 < 3;
 * gamma0, sigma or gamma_snooker not finite; gamma0 < 0. */
int vag_move_propose_dev(vag_ctx* ctx, const vag_move_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop,
                         double* d_factor);
int vag_move_accept_dev(vag_ctx* ctx, const vag_move_spec* sp, uint64_t step, int half, const double* d_prop, const double* d_factor,
                        const double* d_lp_new, double* d_pos, double* d_lp, int64_t* d_accepted);

/* vag_stretch_run_dev with the move mix: steps step0 .. step0 + n_steps - 1 on the likelihood of `request`, per step the choice of
 * the kind, and per half propose, the likelihood call of the n_walkers / 2 proposals, accept.  Buffers, storing, scans, uploads and
 * refusals as there, with the refusals of the building blocks above.  With weights (1, 0, 0) the chain is vag_stretch_run_dev's
 * wherever no decision lies within the rounding of its margin. */
int vag_move_run_dev(vag_ctx* ctx, const vag_loglike_request* request, const vag_move_spec* sp, uint64_t step0, int n_steps,
                     double* d_pos, double* d_lp, int64_t* d_accepted, double* d_chain, double* d_logp);

/* Parallel tempering around the stretch move (added after VAG_ABI_VERSION 13, detect by symbol).
 * The ladder: n_temps = T temperatures, 1 <= T <= VAG_TEMPER_MAX; the inverse temperatures betas[T] are finite, betas[0] = 1,
 * strictly descending, betas[T - 1] >= 0 (0, the prior, is allowed as the last rung).  Temperature t targets
 * ln p_t = betas[t] ln L + ln prior with an ensemble of n_walkers walkers of its own (even, >= 2 ndim, ndim 1 .. 16).  Layouts:
 * pos[T][n_walkers][ndim], lnl[T][n_walkers], lnprior[T][n_walkers], prop[T][n_walkers / 2][ndim], accepted[T][n_walkers],
 * swapped[max(T - 1, 1)][n_walkers].
 * The draws are the stretch move's: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (r, step & 0xffffffff, step >> 32, stream), r = t n_walkers + w the replica's index in the whole ladder, stream 0 the proposal,
 * 1 the acceptance, 2 the exchange; with T = 1 the counters are those of vag_stretch_*_dev.
 * A step is half 0, half 1, then the exchanges.  Half h: every temperature proposes the walkers of its own half h against its own
 * other half exactly as the stretch move does (z and the partner from stream 0, prop = fma(z, pos[t][w] - pos[t][partner],
 * pos[t][partner])).  A proposal whose ln L or ln prior is not finite is rejected at every temperature, beta = 0 included (so every
 * current state has both finite, and the beta = 0 rung is the prior restricted to where the model evaluates); any other is accepted
 * iff log(u_a) < (ndim - 1) log(z) + fma(beta_t, lnl_new - lnl_old, lnprior_new - lnprior_old), u_a from stream 1.  An accepted
 * walker takes the proposal, its ln L and its ln prior, and accepted[t][w] counts one.
 * The exchanges of step s: the pairs (t, t + 1) with t + s even (deterministic even-odd), walker w of t with walker w of t + 1
 * (the walkers of an ensemble are exchangeable: a fixed pairing keeps detailed balance).  With u_s from stream 2 at
 * r = t n_walkers + w the pair exchanges iff log(u_s) < (beta_t - beta_t+1) (lnl[t + 1][w] - lnl[t][w]); it then swaps positions,
 * ln L and ln prior, and swapped[t][w] counts one.  T = 1 has no exchanges.
 * Step s is stored when (s + 1) % thin == 0: the state after the exchanges. */
#define VAG_TEMPER_MAX 64
typedef struct vag_tempered_spec {
    uint64_t seed;
    double a;             /* the stretch scale, finite and > 1 */
    int32_t n_temps;      /* T: 1 .. VAG_TEMPER_MAX */
    int32_t n_walkers;    /* per temperature: even, >= 2 ndim */
    int32_t ndim;         /* 1 .. 16 */
    int32_t thin;         /* >= 1 */
    const double* betas;  /* host, [n_temps] */
} vag_tempered_spec;

/* A likelihood call (the blocks of `request`, as vag_loglike_cov_batch_dev) that returns ln L and ln prior apart, by walker:
 * d_lnl[i] = -chi2 / 2 where the walker was evaluated and its chi^2 is finite, else -inf; d_lnprior[i] the sum of ln prior under
 * spec->use_priors (-inf outside the bounds), else 0.  d_lnl + d_lnprior equals the output of the likelihood entry to the bit
 * wherever that is finite; where that is -inf, at least one of the two is.  Stream-ordered, host-blocking as
 * vag_loglike_batch_dev is. */
int vag_loglike_split_dev(vag_ctx* ctx, const vag_loglike_request* request, const double* d_theta, int nb, int ndim, double* d_lnl,
                          double* d_lnprior);

/* The building blocks (no model), as vag_stretch_propose_dev / vag_stretch_accept_dev: a caller's evaluator of the T n_walkers / 2
 * proposals goes between propose and accept, and swap follows the two halves.  Device pointers, the context's stream, no host
 * synchronisation.  Refused with VAG_E_INVALID (the context stays usable): whatever the stretch entries refuse; n_temps outside
 * 1 .. VAG_TEMPER_MAX (or n_temps n_walkers above 2^30); null betas; betas[0] != 1; a rung that is not finite, not strictly below
 * the one before it, or negative; half not 0 or 1. */
int vag_tempered_propose_dev(vag_ctx* ctx, const vag_tempered_spec* sp, uint64_t step, int half, const double* d_pos, double* d_prop);
int vag_tempered_accept_dev(vag_ctx* ctx, const vag_tempered_spec* sp, uint64_t step, int half, const double* d_prop,
                            const double* d_lnl_new, const double* d_lnprior_new, double* d_pos, double* d_lnl, double* d_lnprior,
                            int64_t* d_accepted);
int vag_tempered_swap_dev(vag_ctx* ctx, const vag_tempered_spec* sp, uint64_t step, double* d_pos, double* d_lnl, double* d_lnprior,
                          int64_t* d_swapped);

/* Steps step0 .. step0 + n_steps - 1 on the likelihood of `request`: per step and half, propose, ONE likelihood call of the
 * T n_walkers / 2 proposals, its split into ln L and ln prior, accept; then the exchanges.  On entry d_lnl / d_lnprior hold those of
 * d_pos, all finite.  The blocks are scanned and uploaded once per call; between the steps there is no copy to the host and no stream
 * synchronisation (a likelihood call itself waits for its device plan).  A stored step writes its row [T][n_walkers][ndim] of
 * d_chain and [T][n_walkers] of d_lnl_chain and d_lnprior_chain, consecutive from the pointers given; all three null: nothing is
 * stored.  n_steps = 0 does nothing.  Refusals as above, and: a null request or request->spec, ndim different from
 * request->spec->ndim, n_steps < 0, the three chain pointers not all null or all set, and whatever the likelihood call refuses. */
int vag_tempered_run_dev(vag_ctx* ctx, const vag_loglike_request* request, const vag_tempered_spec* sp, uint64_t step0, int n_steps,
                         double* d_pos, double* d_lnl, double* d_lnprior, int64_t* d_accepted, int64_t* d_swapped, double* d_chain,
                         double* d_lnl_chain, double* d_lnprior_chain);

/* Nested sampling on the device (added after VAG_ABI_VERSION 13, detect by symbol), by the definition of INTEGRATION.md "Nested
 * sampling".  N = n_live live points, N even, 4 <= N <= VAG_NESTED_MAX_LIVE, ndim 1 .. 16, K = N / 2; every live point has finite
 * ln L and ln prior.  Layouts: live[N][ndim], lnl[N], lnprior[N], order[N] (int32), lstar[1], prop[K][ndim], and per iteration a
 * row of the dead record dead_theta[K][ndim], dead_lnl[K], dead_lnprior[K] and of the counts accepted[K].
 * Iteration `it`: (rank) slot i comes before slot j iff (lnl[i], i) < (lnl[j], j); order[r] is the slot of rank r, the dead are
 * ranks 0 .. K - 1, the survivors ranks K .. N - 1, and lstar[0] = lnl[order[K - 1]].  (retire) The dead row takes the dead in rank
 * order, then slot order[r] becomes a copy of survivor order[K + j0], j0 = floor(u K).  (walk) For m = 1 .. walk: clone r proposes
 * prop[r][d] = fma(gamma, live[s1][d] - live[s2][d], live[order[r]][d]) with the survivors s1 = order[K + a], s2 = order[K + b] and
 * the scale gamma of the DE kind of the move mix above (a, b, n_q, gamma0 = 0 standing for 2.38 / sqrt(2 ndim)); the K proposals in
 * rank order are one likelihood call; clone r takes its proposal iff ln L' and ln prior' are finite, ln L' > lstar[0] (strict) and
 * log(u_a) < ln prior' - ln prior, and accepted[r] counts one.  The survivors do not move during an iteration.
 * The draws are Philox4x32-10 with the key above and counter (r, tick & 0xffffffff, tick >> 32, stream), tick = it (walk + 1) + m:
 * m = 0 the clone draw with u = u(first two words) of stream 5; m = 1 .. walk the walk steps with streams 0 and 4 (the proposal) and
 * 1 (the acceptance) read as the DE kind reads them, nh = K.  The flattened dead record is non-decreasing in ln L; the evidence is
 * formed on the host from it (sampling.nested_evidence). */
#define VAG_NESTED_MAX_LIVE 16384
typedef struct vag_nested_spec {
    uint64_t seed;
    int32_t n_live;  /* N: even, 4 .. VAG_NESTED_MAX_LIVE */
    int32_t ndim;    /* 1 .. 16 */
    int32_t walk;    /* constrained steps per iteration, >= 1 */
    int32_t pad;
    double gamma0;   /* the DE scale, finite and >= 0; 0: the default 2.38 / sqrt(2 ndim) */
    double sigma;    /* the relative jitter of the DE scale, finite (1e-5 is customary) */
} vag_nested_spec;

/* The building blocks (no model): device pointers, the context's stream, no host synchronisation.  rank reads d_lnl and writes
 * d_order and d_lstar; retire writes the dead row given and the dead slots of d_live / d_lnl / d_lnprior; propose writes d_prop;
 * accept reads d_lstar and the proposals' ln L and ln prior, changes the clones in place and adds to d_accepted[K].  m is the walk
 * step, 1 .. walk.  An entry of d_order outside 0 .. N - 1 is read as slot 0.  Refused with VAG_E_INVALID (the context stays usable):
 * a null context, spec or buffer; n_live odd or outside 4 .. VAG_NESTED_MAX_LIVE; ndim outside 1 .. 16; walk < 1; gamma0 not finite
 * or < 0; sigma not finite; m outside 1 .. walk. */
int vag_nested_rank_dev(vag_ctx* ctx, const vag_nested_spec* sp, const double* d_lnl, int32_t* d_order, double* d_lstar);
int vag_nested_retire_dev(vag_ctx* ctx, const vag_nested_spec* sp, uint64_t it, const int32_t* d_order, double* d_live, double* d_lnl,
                          double* d_lnprior, double* d_dead_theta, double* d_dead_lnl, double* d_dead_lnprior);
int vag_nested_propose_dev(vag_ctx* ctx, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_live,
                           double* d_prop);
int vag_nested_accept_dev(vag_ctx* ctx, const vag_nested_spec* sp, uint64_t it, int m, const int32_t* d_order, const double* d_lstar,
                          const double* d_prop, const double* d_lnl_new, const double* d_lnprior_new, double* d_live, double* d_lnl,
                          double* d_lnprior, int64_t* d_accepted);

/* Iterations it0 .. it0 + n_iters - 1 on the likelihood of `request`: per iteration rank, retire, and `walk` times propose, ONE
 * likelihood call of the K proposals, its split into ln L and ln prior, accept.  On entry d_lnl / d_lnprior hold those of d_live,
 * all finite.  Iteration it0 + k fills row k of d_dead_theta[n_iters][K][ndim], d_dead_lnl[n_iters][K], d_dead_lnprior[n_iters][K]
 * and adds to row k of d_accepted[n_iters][K], which the caller zeroes.  The blocks are scanned and uploaded once per call; between
 * the iterations there is no copy to the host and no stream synchronisation (a likelihood call itself waits for its device plan).
 * n_iters = 0 does nothing.  Refusals as above, and: a null request or request->spec, ndim different from request->spec->ndim,
 * n_iters < 0, and whatever the likelihood call refuses. */
int vag_nested_run_dev(vag_ctx* ctx, const vag_loglike_request* request, const vag_nested_spec* sp, uint64_t it0, int n_iters,
                       double* d_live, double* d_lnl, double* d_lnprior, int64_t* d_accepted, double* d_dead_theta, double* d_dead_lnl,
                       double* d_dead_lnprior);

/* Chain autocorrelation on the device (added after VAG_ABI_VERSION 13, detect by symbol): the integrated autocorrelation time of
 * every parameter of a chain in HBM, by the definition of INTEGRATION.md "Chain autocorrelation".
 * The view: n_rows rows, nwalkers walkers, ndim parameters, element (t, w, d) at d_chain[t row_stride + w ndim + d] with
 * row_stride >= nwalkers ndim (a plain chain [rows][W][D]: W D; the cold rung of a tempered chain [rows][T][W][D]: T W D).
 * Per series s = w ndim + d: the two-pass mean m (m1 = (sum x) / n, m = m1 + (sum (x - m1)) / n, ascending t), y = x - m, and
 * c_s(l) = sum_{t <= n - 1 - l} y[t] y[t + l] for l = 0 .. max_lag, one fma chain in ascending t, so its bits depend neither on the
 * launch nor on max_lag.  Pooled over the walkers in ascending w: C_d(l), rho_d(l) = C_d(l) / C_d(0).  Sokal's window:
 * tau_d(M) = 2 sum_{l <= M} rho_d(l) - 1 (a sequential sum), window[d] the smallest M <= max_lag with M >= c tau_d(M) and
 * tau[d] = tau_d(window[d]); if there is none window[d] = -1 and tau[d] = tau_d(max_lag), a lower bound; if C_d(0) is zero or not
 * finite tau[d] = NaN and window[d] = -1, for that parameter alone.  tau is in rows.
 * Device pointers, the context's stream, no host synchronisation; the chain is read only, the outputs are d_rho[max_lag + 1][ndim]
 * (may be NULL), d_tau[ndim], d_window[ndim], and the context's scratch holds the lag sums.
 * Refused with VAG_E_INVALID (nothing is launched, the context stays usable): a null context, spec, chain, tau or window;
 * n_rows < 2; nwalkers < 1 or ndim < 1; row_stride < nwalkers ndim; max_lag outside 1 .. n_rows - 1; c not finite and > 0.
 * Refused with VAG_E_CAPACITY: lag sums (max_lag + 1) nwalkers ndim 8 bytes above VAG_CHAIN_SCRATCH_MAX (1 GiB: 16383 lags of 1024
 * walkers x 8 parameters). */
#define VAG_CHAIN_SCRATCH_MAX (1ll << 30)
typedef struct vag_chain_spec {
    int32_t nwalkers, ndim;
    int64_t n_rows, row_stride;
    int32_t max_lag;
    double c;
} vag_chain_spec;
int vag_chain_autocorr_dev(vag_ctx* ctx, const vag_chain_spec* sp, const double* d_chain, double* d_rho, double* d_tau,
                           int32_t* d_window);

/* Posterior-predictive quantile bands on the device (added after VAG_ABI_VERSION 13, detect by symbol), by the definition of
 * INTEGRATION.md "Posterior-predictive bands" (its pieces as code: csrc/vag_predict.h).
 * Draws F[S][M] in HBM, row s one draw.  A draw is valid when its flag is set (d_valid_in[s] != 0; NULL: every flag set) and all M
 * of its values are finite; n is the number of valid draws, the same for every column.  For each quantile q[k] in [0, 1]:
 * h = q (double)(n - 1) (one FP64 multiply), lo = floor(h), g = h - lo, and with y the column's valid values in ascending order
 * out[k][m] = y[lo] when g == 0, else fma(g, y[lo + 1] - y[lo], y[lo]) -- numpy's default "linear" quantile as a distribution, the
 * rounding fixed here.  A zero of either sign is read as +0.  n == 0: every output is NaN.  Order statistics are exact: the bits of
 * the outputs depend neither on the launch nor on the context.
 * vag_column_quantiles_dev: d_F is only read; outputs d_out[nq][M], d_valid_out[S] (may be NULL) and d_n_valid[1].
 * vag_predict_bands_dev: the S rows of d_theta[S][ndim] go through the transformer of the likelihood (10^theta for log-scale
 * parameters, slot VAG_P_A_V a draw's own A_V, slots above it ignored; no bounds, no priors; the data arrays of spec are not read),
 * the S models through the path of vag_flux_density_grid_batch_dev on the grid d_t[nt] x d_nu[nnu], every flux is multiplied by
 * exp(-A_V d_ext[inu]) where A_V != 0 and d_ext (0.4 ln 10 k(lambda_rest) per frequency, or NULL) is given, and the quantile stage runs
 * on the columns m = inu nt + it.  A draw with a theta that is not finite, or whose model the engine could not evaluate (parameters,
 * grid limits, an ODE row), is invalid and its fluxes are NaN.  Outputs d_bands[nq][nnu][nt], d_draws[S][nnu][nt] (NULL: the
 * context's scratch holds them), d_valid[S] (may be NULL), d_n_valid[1].
 * Both: device pointers, stream-ordered on the context's stream, scratch in the context's grown buffers (the quantile stage itself
 * never waits for the host).  Refused (the context stays usable): VAG_E_INVALID for a null context, spec or required buffer, nq
 * outside 1 .. VAG_PREDICT_MAX_Q, a q outside [0, 1] or NaN, S < 1 or M < 1, ndim other than the spec's, a slot that names no
 * parameter; VAG_E_CAPACITY for S > VAG_PREDICT_MAX_DRAWS or S M > VAG_PREDICT_MAX_VALUES (1 GiB of draws). */
#define VAG_PREDICT_MAX_DRAWS 4096
#define VAG_PREDICT_MAX_Q 16
#define VAG_PREDICT_MAX_VALUES (1ll << 27)
typedef struct vag_quantile_spec {
    int32_t nq;
    int32_t pad;
    double q[VAG_PREDICT_MAX_Q];
} vag_quantile_spec;
int vag_column_quantiles_dev(vag_ctx* ctx, const vag_quantile_spec* qs, const double* d_F, int S, int M, const int32_t* d_valid_in,
                             double* d_out, int32_t* d_valid_out, int32_t* d_n_valid);
int vag_predict_bands_dev(vag_ctx* ctx, const vag_fit_spec* spec, const double* d_theta, int S, int ndim, const double* d_t, int nt,
                          const double* d_nu, int nnu, const double* d_ext, const vag_quantile_spec* qs, double* d_bands,
                          double* d_draws, int32_t* d_valid, int32_t* d_n_valid);

/* Same with theta/out in HBM.  The data arrays of spec are host pointers: their CONTENT is hashed on every call and they are
 * uploaded (one pinned staging copy) only when it differs from the previous call's, so a sampler loop moves no data.
 * Stream-ordered on the context stream, but host-blocking: the call returns after the batch's device plan has been read back
 * (see DESIGN.md "host synchronisation"). */
int vag_loglike_batch_dev(vag_ctx* ctx, const vag_fit_spec* spec, const double* d_theta, int nb, int ndim,
                          double* d_out);

/* Relative cost of every model of the last batch call on this context, into HBM: d_cost[nb] = n_theta * n_phi_eff * n_t, the
 * (theta, phi, t) cell count the equal-arrival-time integration walks (0 for a model that was not evaluated).  Stream-ordered,
 * no host synchronisation.  A sharded sampler balances the next call's walker blocks with it: walker cost varies 8x over a
 * prior box because every walker builds its own adaptive grid (fitter.py:503-533). */
int vag_last_model_costs_dev(vag_ctx* ctx, int nb, double* d_cost);

/*
 * ABI v9 -- one rank's share of a sharded log_prob_batch (the reference spreads eval_one over a thread pool,
 * VegasAfterglow/fitting/samplers.py:72-91; here the walkers are spread over the GPUs of a node, one process per GPU).
 * Every rank holds the SAME d_theta_all[nb_all][ndim] and calls, in this order and without any host work in between:
 *
 *   vag_loglike_shard_dev        deals the walkers on the device -- ranked by the cost the engine reported for them in the previous
 *                                finished call of this size (stable, descending), position q = sweep * world + k goes to rank k on
 *                                even sweeps and world-1-k on odd ones, so every rank gets ceil(nb_all / world) slots (`per`) of
 *                                near-equal total cost --, evaluates this rank's walkers and writes d_block[per][2] =
 *                                {ln L (+ ln prior with use_priors), cost}; padding slots carry {NaN, 0};
 *   <the caller's all-gather>    d_gathered[world * per][2] = the ranks' blocks in rank order (RCCL / any transport);
 *   vag_loglike_shard_finish_dev scatters d_gathered back into walker order, d_out[nb_all], and keeps the gathered costs for the
 *                                next deal (a walker that was not evaluated, cost 0, is assumed average).
 *
 * The deal is a function of the gathered costs only, so all ranks compute the same one without talking.  Stream-ordered on the
 * context stream like vag_loglike_batch_dev; rank / world are the caller's (no communicator is touched here).
 * ABI v11: the deal of a call in flight is kept per (nb_all, world, spec content), so other sharded calls may run on the context between
 * a call's two halves -- a caller need not, and should not, hold a process-local lock across its collective.
 * ABI v13: a call in flight is NAMED.  vag_loglike_shard_begin_dev is vag_loglike_shard_dev plus a ticket (never 0), and
 * vag_loglike_shard_end_dev finishes exactly that call: calls of equal shape may finish in any order, and several calls of the SAME
 * fit may be in flight (each holds its own deal; up to eight in flight on a context, of up to four different (fit, nb_all, world) keys).
 * vag_loglike_shard_end_dev(ctx, ticket, NULL, nb_all, world, NULL) abandons a call (the caller's collective failed): its slot is
 * released and the fit's costs stay as they were.  The unticketed pair stays: its finish takes the OLDEST call in flight of that
 * shape, which is right only while calls of equal shape finish in the order they were dealt, and an unticketed deal of a fit that
 * already has one in flight replaces it.
 */
int vag_loglike_shard_dev(vag_ctx* ctx, const vag_fit_spec* spec, const double* d_theta_all, int nb_all, int ndim, int rank,
                          int world, double* d_block);
int vag_loglike_shard_finish_dev(vag_ctx* ctx, const double* d_gathered, int nb_all, int world, double* d_out);
int vag_loglike_shard_begin_dev(vag_ctx* ctx, const vag_fit_spec* spec, const double* d_theta_all, int nb_all, int ndim, int rank,
                                int world, double* d_block, uint64_t* ticket);
int vag_loglike_shard_end_dev(vag_ctx* ctx, uint64_t ticket, const double* d_gathered, int nb_all, int world, double* d_out);
/* For inspection (either pointer may be NULL): d_table[world * per] = walker of every (rank, slot) in the last deal, -1 = padding;
 * d_cost[nb_all] = the gathered costs the NEXT deal will rank by (after a finished call). */
int vag_loglike_shard_state_dev(vag_ctx* ctx, int nb_all, int world, int32_t* d_table, double* d_cost);

/*
 * Model.details(t_min, t_max) intermediates for ONE model (pybind/pymodel.cpp:315-348):
 * grid sizes first, then arrays copied into caller buffers (any pointer may be NULL).
 *   phi[n_phi], theta[n_theta], t_src[n_theta][n_t] (engine frame, s),
 *   Gamma, r (cm), t_comv (s), B (G), N_p, Gamma_th : [n_theta][n_t]
 */
typedef struct vag_details_shape {
    int32_t n_phi, n_theta, n_t, n_reps;
    int32_t symmetry;     /* 0 structured, 1 phi_symmetric, 2 piecewise, 3 isotropic (src/core/mesh.h:55-60) */
    int32_t phi_mirrored; /* src/core/mesh.h:74-79 */
} vag_details_shape;

typedef struct vag_details_out {
    double* phi;
    double* theta;
    double* t_src;
    double* Gamma;
    double* r;
    double* t_comv;
    double* B;
    double* N_p;
    double* Gamma_th;
} vag_details_out;

int vag_details(vag_ctx* ctx, const vag_model_params* params, double t_min, double t_max, vag_details_shape* shape,
                const vag_details_out* out);
/* Same protocol for the reverse shock of a Model(rvs_rad=...) (Model.details().rvs, pybind/pymodel.cpp:315-348). */
int vag_details_rvs(vag_ctx* ctx, const vag_model_params* params, double t_min, double t_max, vag_details_shape* shape,
                    const vag_details_out* out);
/* ShockDetails' electron / photon arrays of the forward (rvs = 0) or reverse (rvs = 1) shock, each [n_theta][n_t] with the
 * shape vag_details reports (save_electron_details / save_photon_details, pybind/pymodel.cpp:236-290):
 *   arrays[0..10] = gamma_m, gamma_c, gamma_a, gamma_M, N_e, nu_m [Hz], nu_c, nu_a, nu_M, I_nu_max [erg/cm^2/s/Hz], theta.
 * NULL entries are skipped.  With Radiation(ssc=True) these are the inverse-Compton-cooled values. */
int vag_details_radiation(vag_ctx* ctx, const vag_model_params* params, double t_min, double t_max, int rvs,
                          double* const* arrays);
/* ABI v11: SynElectrons::regime of every (theta, t) cell -- determine_regime (src/radiation/synchrotron.cpp:45-60): 1 ... 6 by the
 * ordering of gamma_a, gamma_c, gamma_m, 0 = none -- regime[n_theta][n_t] (shape as vag_details reports it). */
int vag_details_regime(vag_ctx* ctx, const vag_model_params* params, double t_min, double t_max, int rvs, int32_t* regime);
/* ShockDetails.t_obs [s] and .Doppler of every (phi, theta, k) cell (pybind/pymodel.cpp:296-298; shared by the forward
 * and the reverse shock, which ride the same contact discontinuity): [n_phi_eff][n_theta][n_t] with the shape
 * vag_details reports and n_phi_eff = Observer::eff_phi_grid (1 for an on-axis axisymmetric model).  Call with
 * t_obs = doppler = NULL to query n_phi_eff. */
int vag_details_eat(vag_ctx* ctx, const vag_model_params* params, double t_min, double t_max, int* n_phi_eff, double* t_obs,
                    double* doppler);
/* Model.jet_E_iso(phi, theta), Model.jet_Gamma0(phi, theta), Model.medium(phi, theta, r) (pybind.cpp:441-448,
 * pymodel.cpp:572-594) for the named, phi-independent profiles: kind 0 -> isotropic-equivalent energy [erg] at theta[n],
 * 1 -> initial Lorentz factor at theta[n], 2 -> mass density [g/cm^3] at radius r[n] [cm]. */
int vag_profile_eval(vag_ctx* ctx, const vag_model_params* params, int kind, const double* x, int n, double* out);

/* Per-stage device timings (ms) of the last batch call, stage names follow the reference's
 * profiler (pybind/pymodel.h:877-953): grid, dynamics, syn_cells, sync_flux, reduce, total. */
typedef struct vag_stage_times {
    float grid_ms, dynamics_ms, cells_ms, flux_ms, reduce_ms, total_ms;
} vag_stage_times;
int vag_last_stage_times(vag_ctx* ctx, vag_stage_times* out);

/* Per-stage device time of the last call under the reference profiler's stage names (AFTERGLOW_PROFILE_SCOPE in
 * pybind/pymodel.h:877-953; Model.profile_data(), pybind.cpp:458-459), measured with HIP events around the kernels of each
 * stage.  Off by default (every scope costs two event records): vag_ctx_profile(ctx, 1) turns it on for the following calls.
 * What each name covers here, where kernels are fused differently from the reference's loops:
 *   dynamics      adaptive grid + blast-wave ODE (both shocks);
 *   EAT_grid      always 0: the equal-arrival-time logs are recomputed inside the flux kernels (counted in *_flux);
 *   syn_electrons vag_cells_kernel: electrons AND photons of every cell in one pass;
 *   cooling       inverse-Compton cooling recurrence (vag_ic_cooling_kernel);
 *   syn_photons   the photon rebuild from the cooled electrons (vag_photons_ic_kernel; 0 without SSC);
 *   sync_flux     synchrotron flux passes (both shocks) incl. their reductions; the fused synchrotron + SSC pass counts here;
 *   ic_photons    seed band + per-cell SSC spectrum tables;   ssc_flux  SSC flux passes;   total  first to last kernel. */
typedef struct vag_profile {
    double dynamics, EAT_grid, syn_electrons, syn_photons, cooling, sync_flux, ic_photons, ssc_flux, total; /* ms */
} vag_profile;
int vag_ctx_profile(vag_ctx* ctx, int enable);
int vag_last_profile(vag_ctx* ctx, vag_profile* out);

/* Work done by the last batch call, for roofline accounting (SURVEY.md section 8d units):
 *   eat_cells  = sum over models of (theta x phi_eff pairs) x n_t  -- (phi, theta, k) cells of Observer::observe
 *   spec_evals = eat_cells x nnu (grid) or 2 x pairs x n (series)  -- calls of SmoothPowerLawSyn::compute_log2_I_nu
 *   interps    = pairs x nt x nnu (grid) or pairs x n (series)     -- log-log interpolations + exp2 */
typedef struct vag_plan {
    int32_t n_models_ok; /* models whose grid fit the engine limits */
    int32_t n_rows;      /* ODE rows solved (representative theta rows) */
    int64_t n_cells;     /* (row, k) cells = photon parameter blocks */
    int64_t total_pairs; /* (theta, phi_eff) rows integrated by the flux kernel */
    int64_t eat_cells;
    int64_t spec_evals;
    int64_t interps;
    int32_t flux_blocks; /* workgroups of the flux kernel */
    int32_t pairs_per_block;
    int32_t n_models_invalid;  /* parameters rejected by validation (ValueError in the reference) */
    int32_t n_models_capacity; /* adaptive grid larger than the engine limits: NOT evaluated (NaN / -inf) */
    int32_t n_rows_failed;     /* ODE rows without an acceptable step after 500 rejections (error in the reference) */
    int32_t n_rows_gave_up;    /* ODE rows that hit the 100000-step cap or stalled (warning in the reference; row kept) */
    /* ABI v7, likelihood calls only, tallied over ALL passes (point data + every band group) of the last call */
    int32_t n_walkers_rejected;   /* walkers scored -inf: out of bounds, invalid parameters, grid over capacity, failed ODE row, SSC failure, non-finite chi2 */
    int32_t n_walkers_ssc_failed; /* of those: SSC tables over capacity or queried outside their clamped band */
    /* with vag_ctx_count_work(1): the SSC table build's work (ICPhoton::generate_spectrum, inverse-compton.h:529-607), summed over
     * both shocks: ic_terms = sum over cells of (electron-energy nodes x seed-frequency nodes), the accumulation's unit;
     * ic_nodes = sum over cells of (electron + seed + output lattice nodes), the set-up's unit */
    int64_t ic_terms, ic_nodes;
    /* ABI v8: models whose SSC tables were rebuilt over their full theoretical range because a flux pass queried them outside the
     * clamped band (ICPhoton::compute_log2_I_nu's self-healing path, inverse-compton.h:626-635); the pass was then repeated */
    int32_t n_models_ssc_rebuilt;
    /* ABI v11 (the v8 padding word): SSC passes of the last call that had to be repeated with EVERY cell's table because a flux pass
     * queried a cell the lazy selection (tables only for the cells a request's observation window touches) had skipped */
    int32_t n_ssc_all_cell_fallbacks;
    /* ABI v10: bytes of the pool that holds the SSC tables of one shock of the batch (each table as long as its own output lattice;
     * cells no (theta, phi) row queries have none) -- the largest table build of the last call */
    int64_t ic_pool_bytes;
    /* ABI v11, with vag_ctx_count_work(1): right-hand sides the forward-shock solver evaluated for the batch (ForwardShockEqn::operator(),
     * forward-shock.tpp:10-118; FSAL: six per step attempt + one per row); 0 for the solvers that carry no tally (reverse shock,
     * spreading, injection).  In the same mode a likelihood call's spec_evals / interps are tallied by the flux kernel itself
     * (boundary-spectrum evaluations actually formed, data points inside a row's lattice) instead of the 2 / 1 per (row, point) bound. */
    int64_t ode_rhs;
    /* ABI v12: SSC cells of the last call whose lattices exceed the wavefront-per-cell kernel's on-chip layout (more than 128 seed
     * frequencies, 64 electron energies or 192 output nodes) and took the general kernel with its arrays in HBM -- same algorithm, same
     * table.  A likelihood call does not wait for the count: vag_last_plan reads it then, for the call's last table build only */
    int64_t n_ssc_slow_cells;
    /* ABI v13, with vag_ctx_count_work(1): lane utilisation of the forward-shock solver's attempt loop -- live lanes summed over the
     * step attempts of every wavefront / lane slots those attempts occupied (64 per attempt).  A wavefront runs until its slowest row
     * is done (forward-shock.tpp:194-207 loops over rows one by one); the persistent kernel refills finished lanes from a row queue. */
    int64_t ode_lane_attempts, ode_lane_slots;
} vag_plan;
int vag_last_plan(vag_ctx* ctx, vag_plan* out); /* synchronises the stream to read the ODE row counters */
/* Instrumentation: when enabled, grid-flux launches tally the exact spec_evals / interps (window-clamped) with
 * one atomic per workgroup and a host sync; leave disabled in timed runs. */
int vag_ctx_count_work(vag_ctx* ctx, int enable);

/*
 * ABI v11 -- thread pools.  Every entry point that takes a context locks it for its own duration, so a context may be shared by the
 * threads of a pool (the reference releases the GIL in every compute method and its samplers map eval_one over a ThreadPoolExecutor with
 * one Model per thread, pybind/pybind.cpp:424-448, VegasAfterglow/fitting/samplers.py:59-70); calls are served one after the other.
 * The *_coalesced forms take ONE model, block the calling thread, and serve the calls that wait at the same time with the same request
 * (times, frequencies / band) as ONE batch call of the corresponding *_batch entry point: an unmodified thread-pool sampler gets batched
 * throughput.  `out` receives the total ([nnu][nt] / [n] / [nt]); or, with out == NULL, out4[i] != NULL receive the components as in the
 * *_components4_batch forms.  The caller's buffers must stay valid until its call returns; errors are per caller (a batch that fails as
 * a whole is repeated member by member).  Results: the series and band forms are the bits of a single call (their summation tree does
 * not depend on the batch); a grid call's fixed-order sums are laid out per batch, so its values may differ from a single call's in the
 * last bits (~1e-15 relative).
 */
int vag_ctx_coalesce(vag_ctx* ctx, int max_batch /* default 64 */, int wait_us /* the first caller waits this long for company: default 50 */);
int vag_ctx_coalesce_stats(vag_ctx* ctx, long long* calls, long long* batches); /* requests served / batch calls issued so far */
int vag_flux_density_grid_coalesced(vag_ctx* ctx, const vag_model_params* p, const double* t, int nt, const double* nu, int nnu,
                                    double* out, double* const* out4);
int vag_flux_density_coalesced(vag_ctx* ctx, const vag_model_params* p, const double* t, const double* nu, int n, double* out,
                               double* const* out4);
int vag_flux_coalesced(vag_ctx* ctx, const vag_model_params* p, const double* t, int nt, double nu_min, double nu_max, int num_nu,
                       double* out, double* const* out4);

#ifdef __cplusplus
}
#endif
#endif /* VEGASAFTERGLOW_AMD_H */
