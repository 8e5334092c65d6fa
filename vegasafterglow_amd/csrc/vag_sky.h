// Sky images and flux-weighted image moments (Model.sky_image / sky_moments; the definition is the engine's own).
//
// Three kernels per (time chunk of a) request, all in a fixed order of summation:
//   vag_sky_terms_kernel    one wavefront per (theta, phi) row: the row's EAT logs, the bracket of every requested time, the two
//                           boundary spectra of every (nu, t) term with the grid flux pass's evaluators and roundings, the term
//                           exp2(lo + f (hi - lo)) in flux units and its sky-position constants -> a dense term list
//                           [pass][4][image][row] (weight, a, b, c: X = a - b cos phi, Y = c sin phi)
//   vag_sky_deposit_kernel  one wavefront per (image, SKY_TILE^2 pixel tile): the term list in row order, every term split into
//                           its azimuthal parts, the parts that land in the tile added to the tile in LDS with ds_add_f64 (the
//                           lanes of one instruction are applied in lane order, and the tile belongs to one wavefront)
//   vag_sky_moments_kernel  one wavefront per image: F, centroid, central second moments in two passes over the same parts, and
//                           the weight that falls outside the image
// Further consumers of the term list below: visibilities, the visibility groups of the likelihood, and linear polarization (Stokes
// sums and maps, with a second list of what the polarization of a term needs).  DESIGN §4k.
#pragma once
#include "vag_sky_moments.h"

namespace vag {

constexpr int SKY_WAVES = 4;  // rows (wavefronts) per workgroup of the terms kernel
constexpr int SKY_TILE = 64;  // pixels per side of a deposit tile (32 KB of LDS)

struct SkyArgs {
    const vag_model_params* params;  // of the selected emitter (the reverse shock's Radiation for emitter 1)
    const VagGridMeta* meta;
    const double* geo_th;  // [nb][3][th_stride]: cos theta, sin theta, log2 |dcos theta|
    const double* geo_ph;  // [nb][2][ph_stride]: cos phi, log2 dphi
    const int* g_rep_of;
    const long long* cell_off;
    const double* cellpar;  // [rows][VAG_NPAR][n_t] of the selected emitter
    const double* cellq;    // FLUX_SYN_IC
    const double* cellgeo;  // spreading jets: [rows][3][n_t] cos theta, sin theta, log2 |dcos|
    const double* ichdr;    // FLUX_SSC
    const double* icpool;
    int* ic_status;
    const double* sp_table;
    const double* lg2_t_obs;   // [nt] of this chunk
    const double* lg2_nu_obs;  // [nnu]
    int nt, nnu, R;            // R: row stride of the term list (>= n_theta * n_phi_eff of every model)
    int ks;                    // LDS row length (>= every lattice of the batch)
    double* terms;             // [4][nb * nnu * nt][R] of this pass
    double* pol;               // POL: [3][nb * nnu * nt][R] of this pass (u, m0, m1: cos between sight line and radius = m0 + m1 cos phi)
};

// The terms of one (theta, phi) row for every (nu, t) of the chunk.  MODE / SPREAD as in vag_flux_grid_kernel.  POL: also what the
// polarization of a term needs (vag_sky_stokes_kernel), written for the terms of non-zero weight only.
template <int MODE, bool SPREAD, bool POL = false>
__global__ void __launch_bounds__(64 * SKY_WAVES) vag_sky_terms_kernel(SkyArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* s_sp = lds;
    for (int i = threadIdx.x; i < SP_LDS_DOUBLES; i += blockDim.x) s_sp[i] = a.sp_table[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.y, p = blockIdx.x * SKY_WAVES + wave;
    if (p >= a.R) return;
    const VagGridMeta* Mp = a.meta + m;
    const int nt = a.nt, nnu = a.nnu, slots = nt * nnu;
    const size_t G = (size_t)gridDim.y * nnu * nt, plane = G * a.R;
    double* out = a.terms + ((size_t)m * nnu * nt) * a.R + p;  // + (l * nt + idx) * R + comp * plane
    const int n_pairs = Mp->status == 0 ? Mp->n_theta * Mp->n_phi_eff : 0;
    if (p >= n_pairs) {
        for (int s = lane; s < slots; s += 64)
            for (int q = 0; q < 4; ++q) out[(size_t)s * a.R + q * plane] = 0.0;
        return;
    }
    const LdsTab sp_tab = lds_tab(s_sp), lg_tab = lds_tab(s_sp + SP_TABLE_DOUBLES);
    double* s_t = s_sp + SP_LDS_DOUBLES + (size_t)wave * 3 * a.ks;
    double* s_dop = s_t + a.ks;
    double* s_geom = s_dop + a.ks;
    const int n_phi_eff = Mp->n_phi_eff, j = p / n_phi_eff, i = p - j * n_phi_eff;
    const int K = Mp->n_t, ts = Mp->th_stride, ps = Mp->ph_stride;
    const double* gth = a.geo_th + (size_t)m * 3 * ts;
    const double* gph = a.geo_ph + (size_t)m * 2 * ps;
    const int rep = a.g_rep_of[(size_t)m * ts + j] + i * Mp->rep_phi_stride;
    const long long cell0 = a.cell_off[m] + (long long)rep * K;
    const double* row = a.cellpar + cell0 * VAG_NPAR;  // [VAG_NPAR][K]
    const double* geo = SPREAD ? a.cellgeo + cell0 * 3 : nullptr;
    const vag_model_params* Pp = a.params + m;
    const double one_plus_z = 1 + Pp->z;
    const double cos_obs = Mp->cos_obs, sin_obs = Mp->sin_obs;
    // EAT logs of the row: eat_row / eat_row_spread, expression for expression
    const double cos_th = gth[j], sin_th = gth[ts + j], cph = gph[i];
    const double cos_v_row = fma(cos_th, cos_obs, (sin_th * cph) * sin_obs);  // RowGeo::cos_view
    const double t_coeff = (1 - cos_v_row) * (one_plus_z / C_C);
    const double lg2_dOmega = gth[2 * ts + j] + gph[ps + i];
    for (int k = lane; k < K; k += 64) {
        const double G_ = row[VP_GAMMA * K + k], u = row[VP_U * K + k], r = row[VP_R * K + k], teng = row[VP_TENG * K + k];
        const double lr2 = row[VP_LG2_R2 * K + k];
        if constexpr (SPREAD) {
            const double cos_v = geo[K + k] * cph * sin_obs + geo[k] * cos_obs;
            const double lg2_dop = -log2_tab(G_ - u * cos_v, lg_tab);
            const double time = (teng + (1 - cos_v) * r / C_C) * one_plus_z;
            s_dop[k] = lg2_dop;
            s_t[k] = log2_tab(time, lg_tab);
            s_geom[k] = ((geo[2 * K + k] + gph[ps + i]) + lr2) + 3.0 * lg2_dop;
        } else {
            const double lg2_dop = -log2_tab(fma(-u, cos_v_row, G_), lg_tab);
            s_dop[k] = lg2_dop;
            s_t[k] = log2_tab(fma(t_coeff, r, teng * one_plus_z), lg_tab);
            s_geom[k] = (lg2_dOmega + lr2) + 3.0 * lg2_dop;
        }
    }
    wave_sync();
    SpecConst sc;
    sc.init(Pp->p);
    int breach = 0;
    auto boundary = [&](int k, double x) -> double {  // log2 I'(x) + geom_k: the grid flux pass's evaluator for MODE
        if constexpr (MODE == FLUX_SYN) {
            SpecRegs regs;
#pragma unroll
            for (int w = 0; w < 14; ++w) regs.v[w] = row[w * K + k];
            return log2_I_nu_fast(regs, 1, sc, x, sp_tab) + s_geom[k];
        } else if constexpr (MODE == FLUX_SYN_IC) {
            double b0, b1;
            log2_I_nu_ic_pair(row + k, K, a.cellq + cell0 * FLUX_NQ + k, K, sc, x, x, sp_tab, b0, b1);
            return b0 + s_geom[k];
        } else {
            const double* hp = a.ichdr + (size_t)(cell0 + k) * FLUX_IC_HDR;
            const double* tab = a.icpool + (unsigned long long)hp[5];
            return ic_table_eval_hdr(tab, hp[0], hp[1], hp[2], hp[3], hp[4], x, &breach) + s_geom[k];
        }
    };
    const double row_t0 = s_t[0], row_tN = s_t[K - 1];
    const double d_L = Pp->lumi_dist * U_CM;
    const double norm = one_plus_z / (d_L * d_L);
    // a sky angle [rad] per unit radius: 1 / D_A, D_A = d_L / (1 + z)^2 (the observer's own d_L and z, also for the reverse shock)
    const double inv_DA = (one_plus_z * one_plus_z) / d_L;
    for (int s = lane; s < slots; s += 64) {
        const int l = s / nt, idx = s - l * nt;
        const double tq = a.lg2_t_obs[idx];
        double wgt = 0, ca = 0, cb = 0, cc = 0;
        if (tq >= row_t0 && tq < row_tN) {  // a time outside the row's lattice contributes nothing (observer.h:405-433)
            int lo = 0, hi = K - 1;         // s_t[lo] <= tq < s_t[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_t[mid] <= tq)
                    lo = mid;
                else
                    hi = mid;
            }
            const double t_lo = s_t[lo];
            const double f = (tq - t_lo) * (1.0 / (s_t[lo + 1] - t_lo));
            const double nu = a.lg2_nu_obs[l] + Mp->lg2_1pz;
            const double b_lo = boundary(lo, nu - s_dop[lo]), b_hi = boundary(lo + 1, nu - s_dop[lo + 1]);
            const double x = fma(b_hi - b_lo, f, b_lo);
            wgt = (exp2_or_zero(x) * norm) / U_FLUX_DEN_CGS;
            if (wgt != 0) {
                const double lr_lo = log2(row[VP_R * K + lo]), lr_hi = log2(row[VP_R * K + lo + 1]);
                const double rr = exp2(lr_lo + f * (lr_hi - lr_lo)) * inv_DA;
                double ct = cos_th, st = sin_th;
                if constexpr (SPREAD) {
                    const double th_lo = atan2(geo[K + lo], geo[lo]), th_hi = atan2(geo[K + lo + 1], geo[lo + 1]);
                    const double th = th_lo + f * (th_hi - th_lo);
                    ct = cos(th);
                    st = sin(th);
                }
                ca = rr * ct * sin_obs;
                cb = rr * st * cos_obs;
                cc = rr * st;
                if constexpr (POL) {
                    const double u_lo = row[VP_U * K + lo];
                    double* po = a.pol + ((size_t)m * nnu * nt + s) * a.R + p;
                    po[0] = u_lo + f * (row[VP_U * K + lo + 1] - u_lo);
                    po[plane] = ct * cos_obs;
                    po[2 * plane] = st * sin_obs;
                }
            }
        }
        double* o = out + (size_t)s * a.R;
        o[0] = wgt;
        o[plane] = ca;
        o[2 * plane] = cb;
        o[3 * plane] = cc;
    }
    if constexpr (MODE == FLUX_SSC) {
        if (breach) atomicOr(a.ic_status + m, ic_breach_status(breach));
    }
}

// The azimuthal bin of a row's phi node (SkyBin, vag_sky_moments.h).
VAG_DEV SkyBin sky_bin(const VagGridMeta& M, const double* phi, int p, int n_az) {
    SkyBin b;
    const int npe = M.n_phi_eff, i = p % npe, last = npe - 1;
    b.mirrored = false;
    if (npe == 1) {
        b.left = 0.0;
        b.width = 2 * C_PI;
    } else if (M.phi_mirrored) {
        b.mirrored = true;
        b.left = (i > 0) ? 0.5 * (phi[i - 1] + phi[i]) : 0.0;
        const double right = (i < last) ? 0.5 * (phi[i] + phi[i + 1]) : C_PI;
        b.width = right - b.left;
    } else {
        b.left = (i > 0) ? 0.5 * (phi[i - 1] + phi[i]) : phi[0];
        const double right = (i < last) ? 0.5 * (phi[i] + phi[i + 1]) : phi[last];
        b.width = right - b.left;
    }
    b.S = max(1, (int)ceil((double)n_az * b.width / (2 * C_PI)));
    return b;
}

struct SkyImgArgs {
    const VagGridMeta* meta;
    const double* phi;  // [nb][ph_stride]
    const double* terms;
    int n_pass, nnu, nt, R, n_az;
    int nt_all, t0;  // the request's times, first time of this chunk
    double fov;
    int npixel;
    double* image;    // [nb][nnu][nt_all][npixel][npixel] (deposit) or this chunk's [nb * nnu * nt][npixel^2]
    int image_chunk;  // 1: image is the chunk's buffer
    int extra_planes;  // planes that follow every image in `image` (Stokes maps: 2, Q and U)
    double* moments;  // [nb][nnu][nt_all][6] or nullptr
    double* outside;  // [nb][nnu][nt_all] or nullptr
};

VAG_DEV size_t sky_out_index(const SkyImgArgs& a, int g) {  // image g of the chunk -> (m, l, t0 + idx) of the request
    const int idx = g % a.nt, ml = g / a.nt;
    return (size_t)ml * a.nt_all + a.t0 + idx;
}

// One wavefront per (pixel tile, image of the chunk).
__global__ void __launch_bounds__(64) vag_sky_deposit_kernel(SkyImgArgs a) {
    __shared__ double tile[SKY_TILE * SKY_TILE];
    const int lane = threadIdx.x;
    const int g = blockIdx.y, n_tx = (a.npixel + SKY_TILE - 1) / SKY_TILE;
    const int tx0 = (blockIdx.x % n_tx) * SKY_TILE, ty0 = (blockIdx.x / n_tx) * SKY_TILE;
    const int m = g / (a.nnu * a.nt);
    for (int q = lane; q < SKY_TILE * SKY_TILE; q += 64) tile[q] = 0.0;
    wave_sync();
    const VagGridMeta M = a.meta[m];
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const double half = 0.5 * a.fov, delta = a.fov / a.npixel;
    const size_t G = (size_t)gridDim.y, plane = G * a.R;
    // tile bounds in sky coordinates, one pixel wider on every side (a conservative cull; the pixel test below decides)
    const double xlo = (tx0 - 1) * delta - half, xhi = (tx0 + SKY_TILE + 1) * delta - half;
    const double ylo = (ty0 - 1) * delta - half, yhi = (ty0 + SKY_TILE + 1) * delta - half;
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    for (int pass = 0; pass < a.n_pass; ++pass) {
        const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
        for (int r0 = 0; r0 < n_rows; r0 += 64) {
            const int p = r0 + lane;
            double w = 0, ca = 0, cb = 0, cc = 0;
            if (p < n_rows) w = T[p], ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
            if (!(w > 0)) continue;
            if (ca + fabs(cb) < xlo || ca - fabs(cb) > xhi || fabs(cc) < ylo || -fabs(cc) > yhi) continue;
            const SkyBin b = sky_bin(M, phi, p, a.n_az);
            const double part = w / b.S, dphi = b.width / b.S;
            const double wp = b.mirrored ? 0.5 * part : part;
            for (int s = 0; s < b.S; ++s) {
                const double ph = b.left + (s + 0.5) * dphi;
                double sn, cs;
                sincos(ph, &sn, &cs);
                const double X = ca - cb * cs, Y = cc * sn;
                const double fx = floor((X + half) / delta);
                for (int h = 0; h < (b.mirrored ? 2 : 1); ++h) {
                    const double fy = floor(((h ? -Y : Y) + half) / delta);
                    if (fx >= tx0 && fx < tx0 + SKY_TILE && fx < a.npixel && fy >= ty0 && fy < ty0 + SKY_TILE && fy < a.npixel)
                        lds_add_f64(&tile[((int)fy - ty0) * SKY_TILE + ((int)fx - tx0)], wp);
                }
            }
        }
    }
    wave_sync();
    const size_t npix2 = (size_t)a.npixel * a.npixel;
    double* img = a.image + (a.image_chunk ? (size_t)g : sky_out_index(a, g)) * (1 + a.extra_planes) * npix2;
    for (int q = lane; q < SKY_TILE * SKY_TILE; q += 64) {
        const int y = ty0 + q / SKY_TILE, x = tx0 + q % SKY_TILE;
        if (x < a.npixel && y < a.npixel) img[(size_t)y * a.npixel + x] = tile[q];
    }
}

// lane 0 adds the 64 lane values in lane order; every lane gets the sum
VAG_DEV double sky_wave_sum(double v, double* s_red) {
    wave_sync();
    s_red[threadIdx.x] = v;
    wave_sync();
    double t = 0;
    for (int q = 0; q < 64; ++q) t += s_red[q];  // every lane forms the same sum in the same order
    wave_sync();
    return t;
}

// One wavefront per image of the chunk: moments (a.moments) and / or the weight outside the image (a.outside, a.fov > 0).
__global__ void __launch_bounds__(64) vag_sky_moments_kernel(SkyImgArgs a) {
    __shared__ double s_red[64];
    const int lane = threadIdx.x, g = blockIdx.x;
    const int m = g / (a.nnu * a.nt);
    const VagGridMeta M = a.meta[m];
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const size_t G = (size_t)gridDim.x, plane = G * a.R;
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const double half = 0.5 * a.fov, delta = a.fov / a.npixel;
    // visit(fn): every part (weight, X, Y) of this lane's rows, rows in order, parts in order
    auto visit = [&](auto&& fn) {
#pragma unroll 1
        for (int pass = 0; pass < a.n_pass; ++pass) {
            const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
#pragma unroll 1
            for (int p = lane; p < n_rows; p += 64) {
                const double w = T[p];
                if (!(w > 0)) continue;
                const double ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
                const SkyBin b = sky_bin(M, phi, p, a.n_az);
                const double part = w / b.S, dphi = b.width / b.S;
                const double wp = b.mirrored ? 0.5 * part : part;
#pragma unroll 1
                for (int s = 0; s < b.S; ++s) {
                    const double ph = b.left + (s + 0.5) * dphi;
                    double sn, cs;
                    sincos(ph, &sn, &cs);
                    const double X = ca - cb * cs, Y = cc * sn;
                    fn(wp, X, Y);
                    if (b.mirrored) fn(wp, X, -Y);
                }
            }
        }
    };
    double F = 0, SX = 0, SY = 0, out = 0;
    const bool want_out = a.outside != nullptr;
    visit([&](double w, double X, double Y) {
        F += w;
        SX += w * X;
        SY += w * Y;
        if (want_out) {
            const double fx = floor((X + half) / delta), fy = floor((Y + half) / delta);
            if (!(fx >= 0 && fx < a.npixel && fy >= 0 && fy < a.npixel)) out += w;
        }
    });
    F = sky_wave_sum(F, s_red);
    const size_t o = sky_out_index(a, g);
    if (want_out) {
        out = sky_wave_sum(out, s_red);
        if (lane == 0) a.outside[o] = out;
    }
    if (!a.moments) return;
    SX = sky_wave_sum(SX, s_red);
    SY = sky_wave_sum(SY, s_red);
    const double xb = SX / F, yb = SY / F;
    double Sxx = 0, Syy = 0, Sxy = 0;
    visit([&](double w, double X, double Y) {
        const double dx = X - xb, dy = Y - yb;
        Sxx += w * dx * dx;
        Syy += w * dy * dy;
        Sxy += w * dx * dy;
    });
    Sxx = sky_wave_sum(Sxx, s_red);
    Syy = sky_wave_sum(Syy, s_red);
    Sxy = sky_wave_sum(Sxy, s_red);
    if (lane == 0) {
        double* mo = a.moments + o * 6;
        const bool ok = F > 0;
        mo[0] = F;
        mo[1] = ok ? xb : NAN;
        mo[2] = ok ? yb : NAN;
        mo[3] = ok ? Sxx / F : NAN;
        mo[4] = ok ? Syy / F : NAN;
        mo[5] = ok ? Sxy / F : NAN;
    }
}

// ---- visibilities (vag_sky_visibility_batch): a direct Fourier sum over the parts of the term list, no pixels ----
//   vag_sky_visibility_kernel   one wavefront per (image of the chunk, block of 64 baselines, block of SKYV_ROWS of the model's own
//                               rows), lane = baseline: the passes in order, the rows of the block in order, every part in order (+Y
//                               before -Y), V += w exp(-2 pi i (u east + v north)) in registers -> one partial per (row block, image,
//                               baseline)
//   vag_sky_visibility_combine  one thread per (image, baseline): the model's own row blocks in block order
// The row blocks depend on the model's rows only: bitwise reproducible, independent of the batch and of the t-chunking.

constexpr int SKYV_ROWS = 256;  // rows per row block of the visibility kernel

struct SkyVisArgs {
    const VagGridMeta* meta;
    const double* phi;    // [nb][ph_stride]
    const double* terms;  // the term list of this chunk (sky_request)
    const double* u;      // this chunk's baselines [nnu][nt][nbl], wavelengths
    const double* v;
    int n_pass, nnu, nt, R, n_az, nbl;
    double sin_pa, cos_pa;
    double* partial;  // [n_rblk][nb * nnu * nt][nbl][2]
};

__global__ void __launch_bounds__(64) vag_sky_visibility_kernel(SkyVisArgs a) {
    const int lane = threadIdx.x, n_blb = (a.nbl + 63) / 64;
    const int g = blockIdx.x / n_blb, k = (blockIdx.x - g * n_blb) * 64 + lane, rb = blockIdx.y;
    const int m = g / (a.nnu * a.nt), s = g % (a.nnu * a.nt);  // s = l * nt + idx
    const VagGridMeta& M = a.meta[m];
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const int r0 = rb * SKYV_ROWS, r1 = min(n_rows, r0 + SKYV_ROWS);
    if (r0 >= n_rows && r0 > 0) return;  // (the combine reads the blocks of the model's rows only; block 0 always)
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const size_t G = (size_t)gridDim.x / n_blb, plane = G * a.R;
    const bool live = k < a.nbl;
    const double u = live ? a.u[(size_t)s * a.nbl + k] : 0.0, v = live ? a.v[(size_t)s * a.nbl + k] : 0.0;
    const double spa = a.sin_pa, cpa = a.cos_pa;
    double re = 0, im = 0;
    auto add = [&](double w, double X, double Y) {
        const double east = X * spa + Y * cpa, north = X * cpa - Y * spa;
        double sn, cs;
        sincospi(2 * (u * east + v * north), &sn, &cs);
        re += w * cs;
        im -= w * sn;
    };
#pragma unroll 1
    for (int pass = 0; pass < a.n_pass; ++pass) {
        const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
#pragma unroll 1
        for (int p = r0; p < r1; ++p) {  // wave-uniform: every lane reads the same term
            const double w = T[p];
            if (!(w > 0)) continue;
            const double ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
            const SkyBin b = sky_bin(M, phi, p, a.n_az);
            const double part = w / b.S, dphi = b.width / b.S;
            const double wp = b.mirrored ? 0.5 * part : part;
#pragma unroll 1
            for (int q = 0; q < b.S; ++q) {
                const double ph = b.left + (q + 0.5) * dphi;  // vag_sky_deposit_kernel's part, expression for expression
                double sn, cs;
                sincos(ph, &sn, &cs);
                const double X = ca - cb * cs, Y = cc * sn;
                add(wp, X, Y);
                if (b.mirrored) add(wp, X, -Y);
            }
        }
    }
    if (live) {
        double* o = a.partial + (((size_t)rb * G + g) * a.nbl + k) * 2;
        o[0] = re;
        o[1] = im;
    }
}

// One thread per (image of the chunk, baseline): vis [nb * nnu * nt][nbl][2] of the chunk.
__global__ void __launch_bounds__(256) vag_sky_visibility_combine(const VagGridMeta* __restrict__ meta, const double* __restrict__ partial,
                                                                  int G, int nnu, int nt, int nbl, double* __restrict__ vis) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)G * nbl) return;
    const int g = (int)(i / nbl), m = g / (nnu * nt);
    const VagGridMeta M = meta[m];
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const int n_rblk = max(1, (n_rows + SKYV_ROWS - 1) / SKYV_ROWS);
    const size_t blk = (size_t)G * nbl * 2;
    double re = 0, im = 0;
    for (int b = 0; b < n_rblk; ++b) {
        re += partial[b * blk + 2 * i];
        im += partial[b * blk + 2 * i + 1];
    }
    vis[2 * i] = re;
    vis[2 * i + 1] = im;
}

// ---- visibility groups of the likelihood (vag_loglike_vis_batch): the chi^2 of a walker's visibilities, formed in registers ----
//   vag_sky_vis_chi2_kernel   one wavefront per (walker, block of <= 64 visibilities of ONE epoch), lane = visibility: the walker's
//                             own placement from theta, the passes, rows and parts of vag_sky_visibility_kernel in its order (row
//                             blocks of SKYV_ROWS summed on their own, then added in block order, as its combine does), the
//                             baseline-independent part of every azimuthal part (sincos phi, X, Y) formed once per wavefront -- lanes
//                             over parts -- and broadcast by v_readlane, then the residual against the datum and a fixed-order sum
//                             over the wavefront -> one partial chi^2 and one not-finite flag per (walker, visibility block)
// The wavefront walks all rows of its walker: no row-block partials, no V in HBM, and the value depends on the walker alone.

// The walker's sky placement: free parameters with the slots VAG_P_SKY_*, else the fixed values.
VAG_DEV void sky_placement(const double* __restrict__ theta, int walker, int ndim, const double* __restrict__ prior, double& pa,
                           double& e0, double& n0) {
    const int* slot = reinterpret_cast<const int*>(prior + 64);
    const int* is_log = slot + 16;
    for (int d = 0; d < ndim; ++d) {
        const int sl = slot[d];
        if (sl < VAG_P_SKY_PA || sl > VAG_P_SKY_NORTH0) continue;
        const double v = theta[(size_t)walker * ndim + d];
        const double val = is_log[d] ? pow(10.0, v) : v;
        pa = sl == VAG_P_SKY_PA ? val : pa;  // (selects: an if chain becomes an indexed store to scratch)
        e0 = sl == VAG_P_SKY_EAST0 ? val : e0;
        n0 = sl == VAG_P_SKY_NORTH0 ? val : n0;
    }
}

// lane j's value in every lane (j wave-uniform)
VAG_DEV double wave_bcast(double v, int j) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

struct SkyVisFitArgs {
    const VagGridMeta* meta;
    const double* phi;     // [nb][ph_stride]
    const double* terms;   // the term list of this chunk of epochs: [pass][4][nb * nt][R]
    const double* theta;   // [nb][ndim] sampler space
    const double* prior;   // the fit spec's prior block (slot map behind it)
    const int* order;      // evaluation slot -> walker, or null
    const double* obs;     // the group's [u | v | re | im | err | weight], n_vis each
    const int* blocks;     // [n_blk_all][3]: epoch, first visibility, visibilities (<= 64) of every block, epochs ascending
    double pa_fixed, east0_fixed, north0_fixed;
    int ndim, n_vis, n_blk_all;
    int blk0, n_blk;  // the blocks of this chunk's epochs
    int t0, nt;       // this chunk's epochs t0 .. t0 + nt - 1
    int n_pass, R, n_az, kind;
    double* partial;  // [nb][n_blk_all][2]: chi^2 of the block, 1.0 when a V_mod of the block is not finite
};

__global__ void __launch_bounds__(64) vag_sky_vis_chi2_kernel(SkyVisFitArgs a) {
    const int lane = threadIdx.x;
    const int m = blockIdx.x / a.n_blk, blk = a.blk0 + (int)(blockIdx.x - (unsigned)m * a.n_blk);
    const int nb = gridDim.x / a.n_blk;
    const int e = a.blocks[3 * blk], k0 = a.blocks[3 * blk + 1], cnt = a.blocks[3 * blk + 2];
    const int g = m * a.nt + (e - a.t0);  // image of the chunk
    const VagGridMeta& M = a.meta[m];
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const size_t G = (size_t)nb * a.nt, plane = G * a.R;
    const bool live = lane < cnt;
    const int k = live ? k0 + lane : k0;
    const size_t nv = (size_t)a.n_vis;
    const double u = a.obs[k], v = a.obs[nv + k];
    double pa = a.pa_fixed, e0 = a.east0_fixed, n0 = a.north0_fixed;
    sky_placement(a.theta, a.order ? a.order[m] : m, a.ndim, a.prior, pa, e0, n0);
    double spa, cpa;
    sincos(pa, &spa, &cpa);
    double re = 0, im = 0, re_b = 0, im_b = 0;
    auto add = [&](double w, double X, double Y) {  // vag_sky_visibility_kernel's
        const double east = X * spa + Y * cpa, north = X * cpa - Y * spa;
        double sn, cs;
        sincospi(2 * (u * east + v * north), &sn, &cs);
        re_b += w * cs;
        im_b -= w * sn;
    };
#pragma unroll 1
    for (int r0 = 0; r0 < n_rows; r0 += SKYV_ROWS) {
        const int r1 = min(n_rows, r0 + SKYV_ROWS);
        re_b = 0, im_b = 0;
#pragma unroll 1
        for (int pass = 0; pass < a.n_pass; ++pass) {
            const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
#pragma unroll 1
            for (int p = r0; p < r1; ++p) {  // wave-uniform: every lane reads the same term
                const double w = T[p];
                if (!(w > 0)) continue;
                const double ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
                const SkyBin b = sky_bin(M, phi, p, a.n_az);
                const double part = w / b.S, dphi = b.width / b.S;
                const double wp = b.mirrored ? 0.5 * part : part;
#pragma unroll 1
                for (int q0 = 0; q0 < b.S; q0 += 64) {
                    const double ph = b.left + ((q0 + lane) + 0.5) * dphi;  // lane = part: vag_sky_deposit_kernel's part
                    double sn, cs;
                    sincos(ph, &sn, &cs);
                    const double X = ca - cb * cs, Y = cc * sn;
                    const int nq = min(64, b.S - q0);
#pragma unroll 1
                    for (int j = 0; j < nq; ++j) {  // lane = visibility again: the parts in order
                        const double Xj = wave_bcast(X, j), Yj = wave_bcast(Y, j);
                        add(wp, Xj, Yj);
                        if (b.mirrored) add(wp, Xj, -Yj);
                    }
                }
            }
        }
        re += re_b;
        im += im_b;
    }
    double term = 0;
    bool bad = false;
    if (live) {
        const double o_re = a.obs[2 * nv + k], err = a.obs[4 * nv + k], wk = a.obs[5 * nv + k];
        bad = !isfinite(re) || !isfinite(im);
        double r2;
        if (a.kind == VAG_VIS_AMPLITUDE) {
            const double d = o_re - hypot(re, im);
            r2 = d * d;
        } else {
            double sn, cs;  // exp(-2 pi i (u east0 + v north0))
            sincospi(-2 * (u * e0 + v * n0), &sn, &cs);
            const double dr = o_re - (re * cs - im * sn), di = a.obs[3 * nv + k] - (re * sn + im * cs);
            r2 = dr * dr + di * di;
        }
        term = wk * r2 / (err * err);
    }
    term = wave_sum(term);
    const bool any_bad = __any(bad);
    if (lane == 0) {
        double* o = a.partial + ((size_t)m * a.n_blk_all + blk) * 2;
        o[0] = term;
        o[1] = any_bad ? 1.0 : 0.0;
    }
}

// ---- exact centroids (vag_sky_centroid_batch and the likelihood's centroid groups): no term list, no azimuthal parts ----
//   vag_sky_centroid_kernel   one (theta, phi) row per lane, 64 rows per wavefront: the row's EAT logs, bracket and boundary spectra
//                             with vag_sky_terms_kernel's expressions, the term (w, a, b, c), its exact moments over the row's phi bin
//                             (sky_term_moments), and a fixed butterfly of Chan updates over the wavefront -> one partial per
//                             (pass, model, (nu, t) slot, block of 64 rows)
//   vag_sky_centroid_combine  one thread per (model, slot): the partials in pass order, then block order -> F, centroid, moments
// Both orders are fixed and a model's result depends on its own rows only: bitwise reproducible and independent of the batch.

constexpr int SKYC_WAVES = 4;  // blocks of 64 rows (wavefronts) per workgroup
constexpr int SKYC_ROWS = 64;

struct SkyCenArgs {
    const vag_model_params* params;  // of the selected emitter
    const VagGridMeta* meta;
    const double* geo_th;
    const double* geo_ph;
    const double* phi;  // [nb][ph_stride]
    const int* g_rep_of;
    const long long* cell_off;
    const double* cellpar;
    const double* cellq;
    const double* cellgeo;
    const double* ichdr;
    const double* icpool;
    int* ic_status;
    const double* sp_table;
    const double* lg2_t_obs;   // [nt] of this chunk
    const double* lg2_nu_obs;  // [nnu]
    int nt, nnu, n_blk;        // n_blk: blocks of 64 rows per model in the partial layout (>= every model's)
    double* partial;           // this pass's [nb][nnu * nt][n_blk][6]
};

VAG_DEV SkyMom sky_mom_shfl_xor(const SkyMom& v, int off) {
    SkyMom r;
    r.w = __shfl_xor(v.w, off, 64);
    r.x = __shfl_xor(v.x, off, 64);
    r.y = __shfl_xor(v.y, off, 64);
    r.mxx = __shfl_xor(v.mxx, off, 64);
    r.myy = __shfl_xor(v.myy, off, 64);
    r.mxy = __shfl_xor(v.mxy, off, 64);
    return r;
}

template <int MODE, bool SPREAD>
__global__ void __launch_bounds__(SKYC_ROWS * SKYC_WAVES) vag_sky_centroid_kernel(SkyCenArgs a) {
    __shared__ double s_sp[SP_LDS_DOUBLES];
    for (int i = threadIdx.x; i < SP_LDS_DOUBLES; i += blockDim.x) s_sp[i] = a.sp_table[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.y, vb = blockIdx.x * SKYC_WAVES + wave;
    const VagGridMeta* Mp = a.meta + m;
    const int n_pairs = Mp->status == 0 ? Mp->n_theta * Mp->n_phi_eff : 0;
    if (vb * SKYC_ROWS >= n_pairs) return;  // (the combine reads the blocks of live rows only)
    const LdsTab sp_tab = lds_tab(s_sp), lg_tab = lds_tab(s_sp + SP_TABLE_DOUBLES);
    const int nt = a.nt, slots = nt * a.nnu;
    const bool live = vb * SKYC_ROWS + lane < n_pairs;
    const int p = live ? vb * SKYC_ROWS + lane : n_pairs - 1;
    const int n_phi_eff = Mp->n_phi_eff, j = p / n_phi_eff, i = p - j * n_phi_eff;
    const int K = Mp->n_t, ts = Mp->th_stride, ps = Mp->ph_stride;
    const double* gth = a.geo_th + (size_t)m * 3 * ts;
    const double* gph = a.geo_ph + (size_t)m * 2 * ps;
    const int rep = a.g_rep_of[(size_t)m * ts + j] + i * Mp->rep_phi_stride;
    const long long cell0 = a.cell_off[m] + (long long)rep * K;
    const double* row = a.cellpar + cell0 * VAG_NPAR;  // [VAG_NPAR][K]
    const double* geo = SPREAD ? a.cellgeo + cell0 * 3 : nullptr;
    const vag_model_params* Pp = a.params + m;
    const double one_plus_z = 1 + Pp->z;
    const double cos_obs = Mp->cos_obs, sin_obs = Mp->sin_obs;
    const double cos_th = gth[j], sin_th = gth[ts + j], cph = gph[i];
    const double cos_v_row = fma(cos_th, cos_obs, (sin_th * cph) * sin_obs);  // RowGeo::cos_view
    const double t_coeff = (1 - cos_v_row) * (one_plus_z / C_C);
    const double lg2_dOmega = gth[2 * ts + j] + gph[ps + i];
    // node k of the row: log2 t_obs, log2 Doppler, log2 (dOmega r^2 D^3) -- vag_sky_terms_kernel's staged values, expression for expression
    auto node_t = [&](int k) -> double {
        const double u = row[VP_U * K + k], r = row[VP_R * K + k], teng = row[VP_TENG * K + k];
        if constexpr (SPREAD) {
            const double cos_v = geo[K + k] * cph * sin_obs + geo[k] * cos_obs;
            return log2_tab((teng + (1 - cos_v) * r / C_C) * one_plus_z, lg_tab);
        } else {
            (void)u;
            return log2_tab(fma(t_coeff, r, teng * one_plus_z), lg_tab);
        }
    };
    auto node_dop_geom = [&](int k, double& dop, double& geom) {
        const double G_ = row[VP_GAMMA * K + k], u = row[VP_U * K + k], lr2 = row[VP_LG2_R2 * K + k];
        if constexpr (SPREAD) {
            const double cos_v = geo[K + k] * cph * sin_obs + geo[k] * cos_obs;
            dop = -log2_tab(G_ - u * cos_v, lg_tab);
            geom = ((geo[2 * K + k] + gph[ps + i]) + lr2) + 3.0 * dop;
        } else {
            dop = -log2_tab(fma(-u, cos_v_row, G_), lg_tab);
            geom = (lg2_dOmega + lr2) + 3.0 * dop;
        }
    };
    SpecConst sc;
    sc.init(Pp->p);
    int breach = 0;
    auto boundary = [&](int k, double x) -> double {  // log2 I'(x) without geom: the grid flux pass's evaluator for MODE
        if constexpr (MODE == FLUX_SYN) {
            SpecRegs regs;
#pragma unroll
            for (int w = 0; w < 14; ++w) regs.v[w] = row[w * K + k];
            return log2_I_nu_fast(regs, 1, sc, x, sp_tab);
        } else if constexpr (MODE == FLUX_SYN_IC) {
            double b0, b1;
            log2_I_nu_ic_pair(row + k, K, a.cellq + cell0 * FLUX_NQ + k, K, sc, x, x, sp_tab, b0, b1);
            return b0;
        } else {
            const double* hp = a.ichdr + (size_t)(cell0 + k) * FLUX_IC_HDR;
            const double* tab = a.icpool + (unsigned long long)hp[5];
            return ic_table_eval_hdr(tab, hp[0], hp[1], hp[2], hp[3], hp[4], x, &breach);
        }
    };
    const double row_t0 = node_t(0), row_tN = node_t(K - 1);
    const double d_L = Pp->lumi_dist * U_CM;
    const double norm = one_plus_z / (d_L * d_L);
    const double inv_DA = (one_plus_z * one_plus_z) / d_L;
    const SkyBin bin = sky_bin(*Mp, a.phi + (size_t)m * ps, p, 1);
    double* out = a.partial + ((size_t)m * slots * a.n_blk + vb) * 6;
#pragma unroll 1
    for (int s = 0; s < slots; ++s) {
        const int l = s / nt, idx = s - l * nt;
        const double tq = a.lg2_t_obs[idx];
        SkyMom r{0, 0, 0, 0, 0, 0};
        if (live && tq >= row_t0 && tq < row_tN) {
            int lo = 0, hi = K - 1;  // t[lo] <= tq < t[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (node_t(mid) <= tq)
                    lo = mid;
                else
                    hi = mid;
            }
            const double t_lo = node_t(lo);
            const double f = (tq - t_lo) * (1.0 / (node_t(lo + 1) - t_lo));
            const double nu = a.lg2_nu_obs[l] + Mp->lg2_1pz;
            double dop_lo, geom_lo, dop_hi, geom_hi;
            node_dop_geom(lo, dop_lo, geom_lo);
            node_dop_geom(lo + 1, dop_hi, geom_hi);
            const double b_lo = boundary(lo, nu - dop_lo) + geom_lo, b_hi = boundary(lo + 1, nu - dop_hi) + geom_hi;
            const double x = fma(b_hi - b_lo, f, b_lo);
            const double wgt = (exp2_or_zero(x) * norm) / U_FLUX_DEN_CGS;
            if (wgt != 0) {
                const double lr_lo = log2(row[VP_R * K + lo]), lr_hi = log2(row[VP_R * K + lo + 1]);
                const double rr = exp2(lr_lo + f * (lr_hi - lr_lo)) * inv_DA;
                double ct = cos_th, st = sin_th;
                if constexpr (SPREAD) {
                    const double th_lo = atan2(geo[K + lo], geo[lo]), th_hi = atan2(geo[K + lo + 1], geo[lo + 1]);
                    const double th = th_lo + f * (th_hi - th_lo);
                    ct = cos(th);
                    st = sin(th);
                }
                r = sky_term_moments(wgt, rr * ct * sin_obs, rr * st * cos_obs, rr * st, bin);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {  // the lower lane's set first: both lanes of a pair hold the same result
            const SkyMom q = sky_mom_shfl_xor(r, off);
            r = (lane & off) ? sky_mom_merge(q, r) : sky_mom_merge(r, q);
        }
        if (lane == 0) {
            double* o = out + (size_t)s * a.n_blk * 6;
            o[0] = r.w;
            o[1] = r.x;
            o[2] = r.y;
            o[3] = r.mxx;
            o[4] = r.myy;
            o[5] = r.mxy;
        }
    }
    if constexpr (MODE == FLUX_SSC) {
        if (breach) atomicOr(a.ic_status + m, ic_breach_status(breach));
    }
}

// One thread per (model, slot) of the chunk: moments [nb][nnu][nt_all][6] (F, Xbar, Ybar, varX, varY, covXY; F <= 0 or NaN: NaN shape).
__global__ void __launch_bounds__(256) vag_sky_centroid_combine(const VagGridMeta* __restrict__ meta, const double* __restrict__ partial,
                                                                int n_pass, int nb, int nnu, int nt, int n_blk, int nt_all, int t0,
                                                                double* __restrict__ moments) {
    const int slots = nnu * nt;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nb * slots) return;
    const int m = g / slots, s = g - m * slots, l = s / nt, idx = s - l * nt;
    const VagGridMeta M = meta[m];
    const int n_pairs = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const int nblk_m = (n_pairs + SKYC_ROWS - 1) / SKYC_ROWS;
    const size_t pass_stride = (size_t)nb * slots * n_blk * 6;
    SkyMom r{0, 0, 0, 0, 0, 0};
    for (int q = 0; q < n_pass; ++q) {
        const double* P = partial + q * pass_stride + ((size_t)g * n_blk) * 6;
        for (int b = 0; b < nblk_m; ++b) {
            const double* o = P + (size_t)b * 6;
            r = sky_mom_merge(r, SkyMom{o[0], o[1], o[2], o[3], o[4], o[5]});
        }
    }
    double* mo = moments + (((size_t)m * nnu + l) * nt_all + t0 + idx) * 6;
    const bool ok = r.w > 0;
    mo[0] = r.w;
    mo[1] = ok ? r.x : NAN;
    mo[2] = ok ? r.y : NAN;
    mo[3] = ok ? r.mxx / r.w : NAN;
    mo[4] = ok ? r.myy / r.w : NAN;
    mo[5] = ok ? r.mxy / r.w : NAN;
}

// ---- linear polarization (vag_sky_polarization_batch / vag_sky_stokes_image_batch; the definition: INTEGRATION.md, "Polarization") ----
//   vag_sky_stokes_kernel          one wavefront per (block of SKYP_ROWS of the model's own rows, image of the chunk), lane = row: the
//                                  passes in order, the row's parts in order, I, Q, U (and their shares outside the image) in
//                                  registers, a fixed-order sum over the wavefront -> one partial per (row block, image)
//   vag_sky_stokes_combine         one thread per image: the model's own row blocks in block order, then the turn by 2 pa
//   vag_sky_stokes_deposit_kernel  vag_sky_deposit_kernel for the signed planes Q and U (blockIdx.z); the I plane is that kernel's
// A synchrotron pass carries the polarization of its emitter; an SSC pass adds to I only.  The row blocks depend on the model's rows
// only: bitwise reproducible, independent of the batch and of the t-chunking.

constexpr int SKYP_ROWS = 64;  // rows per row block of the Stokes kernel (one per lane)

struct SkyPolArgs {
    const VagGridMeta* meta;
    const double* phi;    // [nb][ph_stride]
    const double* terms;  // the term list of this chunk (sky_request)
    const double* pol;    // its polarization list [pass][3][image][row]
    const double* spec;   // [nb][4]: b - 1 of the forward, reverse shock, Pi_max of the forward, reverse shock
    int pass_em[4];       // the emitter of every pass, -1: unpolarized (SSC)
    int n_pass, nnu, nt, R, n_az;
    int nt_all, t0;
    double fov;  // > 0: also the Stokes sums outside the image of npixel^2 pixels
    int npixel;
    double sin_2pa, cos_2pa;
    double* partial;  // [n_rblk][nb * nnu * nt][6]: I, Q, U, then the same outside the image
    double* stokes;   // [nb][nnu][nt_all][3] on the sky, or nullptr
    double* outside;  // [nb][nnu][nt_all][3] in the jet frame, or nullptr
};

// what is per term in the polarization of its parts
struct SkyPolTerm {
    double u, Gam, m0, m1, kb;  // Gamma beta, Gamma, mu = m0 + m1 cos phi, b - 1
    double pw;                  // Pi_max times the weight of a part
};

VAG_DEV SkyPolTerm sky_pol_term(const double* P, size_t plane, int p, double kb, double pi_max, double part) {
    SkyPolTerm t;
    t.u = P[p];
    t.m0 = P[plane + p];
    t.m1 = P[2 * plane + p];
    t.Gam = sqrt(fma(t.u, t.u, 1.0));
    t.kb = kb;
    t.pw = pi_max * part;
    return t;
}

// Q and U of one part of full weight at (X, Y), cs = cos phi of the part: two divisions, no atan2.
//   s = sin^2 theta' = (1 - mu^2) / (Gamma - u mu)^2,  Pi = Pi_max (b - 1) s / (2 + (b - 1) s),
//   Q = -Pi w cos 2psi, U = -Pi w sin 2psi with cos 2psi = (X^2 - Y^2) / (X^2 + Y^2), sin 2psi = 2 X Y / (X^2 + Y^2)
VAG_DEV void sky_part_qu(const SkyPolTerm& t, double cs, double X, double Y, double& qv, double& uv) {
    const double mu = fma(t.m1, cs, t.m0);
    const double den = fma(-t.u, mu, t.Gam);
    const double sv = dmin(dmax(fma(-mu, mu, 1.0) / (den * den), 0.0), 1.0);
    const double ks = t.kb * sv;  // >= -1
    const double xx = X * X, yy = Y * Y, r2 = xx + yy;
    qv = 0.0, uv = 0.0;
    if (r2 > 0) {
        const double f = -t.pw * (ks / ((2.0 + ks) * r2));
        qv = f * (xx - yy);
        uv = f * (2 * (X * Y));
    }
}

__global__ void __launch_bounds__(64) vag_sky_stokes_kernel(SkyPolArgs a) {
    const int lane = threadIdx.x, g = blockIdx.x, rb = blockIdx.y;
    const int m = g / (a.nnu * a.nt);
    const VagGridMeta& M = a.meta[m];
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    if (rb * SKYP_ROWS >= n_rows && rb > 0) return;  // (the combine reads the blocks of the model's rows only; block 0 always)
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const size_t G = (size_t)gridDim.x, plane = G * a.R;
    const int p = rb * SKYP_ROWS + lane;
    const bool live = p < n_rows;
    const bool want_out = a.fov > 0;
    const double half = 0.5 * a.fov, delta = a.fov / a.npixel;
    auto is_out = [&](double X, double Y) {
        const double fx = floor((X + half) / delta), fy = floor((Y + half) / delta);
        return !(fx >= 0 && fx < a.npixel && fy >= 0 && fy < a.npixel);
    };
    SkyBin b{0.0, 0.0, 0, false};
    if (live) b = sky_bin(M, phi, p, a.n_az);
    const double dphi = live ? b.width / b.S : 0.0;
    double sI = 0, sQ = 0, sU = 0, oI = 0, oQ = 0, oU = 0;
#pragma unroll 1
    for (int pass = 0; pass < a.n_pass; ++pass) {
        const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
        const double w = live ? T[p] : 0.0;
        if (!(w > 0)) continue;
        const double ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
        const double part = w / b.S;
        const int em = a.pass_em[pass];  // wave-uniform
        SkyPolTerm t{0, 1, 0, 0, 0, 0};
        if (em >= 0)
            t = sky_pol_term(a.pol + (size_t)pass * 3 * plane + (size_t)g * a.R, plane, p, a.spec[4 * m + em], a.spec[4 * m + 2 + em], part);
#pragma unroll 1
        for (int s = 0; s < b.S; ++s) {
            const double ph = b.left + (s + 0.5) * dphi;  // vag_sky_deposit_kernel's part, expression for expression
            double sn, cs;
            sincos(ph, &sn, &cs);
            const double X = ca - cb * cs, Y = cc * sn;
            double qv = 0, uv = 0;
            if (em >= 0) sky_part_qu(t, cs, X, Y, qv, uv);
            sI += part;
            sQ += qv;
            if (b.mirrored) {  // the halves at +Y and -Y together: Q of the whole part, no U
                if (want_out) {
                    const bool o_hi = is_out(X, Y), o_lo = is_out(X, -Y);
                    if (o_hi) oI += 0.5 * part, oQ += 0.5 * qv, oU += 0.5 * uv;
                    if (o_lo) oI += 0.5 * part, oQ += 0.5 * qv, oU -= 0.5 * uv;
                }
            } else {
                sU += uv;
                if (want_out && is_out(X, Y)) oI += part, oQ += qv, oU += uv;
            }
        }
    }
    sI = wave_sum(sI);
    sQ = wave_sum(sQ);
    sU = wave_sum(sU);
    if (want_out) {
        oI = wave_sum(oI);
        oQ = wave_sum(oQ);
        oU = wave_sum(oU);
    }
    if (lane == 0) {
        double* o = a.partial + ((size_t)rb * G + g) * 6;
        o[0] = sI, o[1] = sQ, o[2] = sU, o[3] = oI, o[4] = oQ, o[5] = oU;
    }
}

// One thread per image of the chunk.
__global__ void __launch_bounds__(256) vag_sky_stokes_combine(SkyPolArgs a, int G) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int m = g / (a.nnu * a.nt);
    const VagGridMeta M = a.meta[m];
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    const int n_rblk = max(1, (n_rows + SKYP_ROWS - 1) / SKYP_ROWS);
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (int b = 0; b < n_rblk; ++b) {
        const double* o = a.partial + ((size_t)b * G + g) * 6;
#pragma unroll
        for (int q = 0; q < 6; ++q) v[q] += o[q];
    }
    const int idx = g % a.nt, ml = g / a.nt;
    const size_t o = ((size_t)ml * a.nt_all + a.t0 + idx) * 3;
    if (a.stokes) {
        a.stokes[o] = v[0];
        a.stokes[o + 1] = v[1] * a.cos_2pa - v[2] * a.sin_2pa;
        a.stokes[o + 2] = v[1] * a.sin_2pa + v[2] * a.cos_2pa;
    }
    if (a.outside) a.outside[o] = v[3], a.outside[o + 1] = v[4], a.outside[o + 2] = v[5];
}

// One wavefront per (pixel tile, image of the chunk, plane Q or U): vag_sky_deposit_kernel's walk and tile, the value of a part its
// Q or U (half of it at +Y and at -Y on a mirrored grid, U with the sign of Y).  a.image is the chunk's [image][3][npixel^2].
__global__ void __launch_bounds__(64) vag_sky_stokes_deposit_kernel(SkyImgArgs a, SkyPolArgs pa) {
    __shared__ double tile[SKY_TILE * SKY_TILE];
    const int lane = threadIdx.x;
    const int g = blockIdx.y, n_tx = (a.npixel + SKY_TILE - 1) / SKY_TILE;
    const int tx0 = (blockIdx.x % n_tx) * SKY_TILE, ty0 = (blockIdx.x / n_tx) * SKY_TILE;
    const bool want_u = blockIdx.z == 1;
    const int m = g / (a.nnu * a.nt);
    for (int q = lane; q < SKY_TILE * SKY_TILE; q += 64) tile[q] = 0.0;
    wave_sync();
    const VagGridMeta M = a.meta[m];
    const double* phi = a.phi + (size_t)m * M.ph_stride;
    const double half = 0.5 * a.fov, delta = a.fov / a.npixel;
    const size_t G = (size_t)gridDim.y, plane = G * a.R;
    const double xlo = (tx0 - 1) * delta - half, xhi = (tx0 + SKY_TILE + 1) * delta - half;
    const double ylo = (ty0 - 1) * delta - half, yhi = (ty0 + SKY_TILE + 1) * delta - half;
    const int n_rows = M.status == 0 ? M.n_theta * M.n_phi_eff : 0;
    for (int pass = 0; pass < a.n_pass; ++pass) {
        const int em = pa.pass_em[pass];
        if (em < 0) continue;
        const double* T = a.terms + (size_t)pass * 4 * plane + (size_t)g * a.R;
        const double* P = pa.pol + (size_t)pass * 3 * plane + (size_t)g * a.R;
        for (int r0 = 0; r0 < n_rows; r0 += 64) {
            const int p = r0 + lane;
            double w = 0, ca = 0, cb = 0, cc = 0;
            if (p < n_rows) w = T[p], ca = T[plane + p], cb = T[2 * plane + p], cc = T[3 * plane + p];
            if (!(w > 0)) continue;
            if (ca + fabs(cb) < xlo || ca - fabs(cb) > xhi || fabs(cc) < ylo || -fabs(cc) > yhi) continue;
            const SkyBin b = sky_bin(M, phi, p, a.n_az);
            const double part = w / b.S, dphi = b.width / b.S;
            const SkyPolTerm t = sky_pol_term(P, plane, p, pa.spec[4 * m + em], pa.spec[4 * m + 2 + em], part);
            for (int s = 0; s < b.S; ++s) {
                const double ph = b.left + (s + 0.5) * dphi;
                double sn, cs;
                sincos(ph, &sn, &cs);
                const double X = ca - cb * cs, Y = cc * sn;
                double qv, uv;
                sky_part_qu(t, cs, X, Y, qv, uv);
                const double val = b.mirrored ? 0.5 * (want_u ? uv : qv) : (want_u ? uv : qv);
                const double fx = floor((X + half) / delta);
                for (int h = 0; h < (b.mirrored ? 2 : 1); ++h) {
                    const double fy = floor(((h ? -Y : Y) + half) / delta);
                    if (fx >= tx0 && fx < tx0 + SKY_TILE && fx < a.npixel && fy >= ty0 && fy < ty0 + SKY_TILE && fy < a.npixel)
                        lds_add_f64(&tile[((int)fy - ty0) * SKY_TILE + ((int)fx - tx0)], (h && want_u) ? -val : val);
                }
            }
        }
    }
    wave_sync();
    const size_t npix2 = (size_t)a.npixel * a.npixel;
    double* img = a.image + ((size_t)g * 3 + 1 + blockIdx.z) * npix2;
    for (int q = lane; q < SKY_TILE * SKY_TILE; q += 64) {
        const int y = ty0 + q / SKY_TILE, x = tx0 + q % SKY_TILE;
        if (x < a.npixel && y < a.npixel) img[(size_t)y * a.npixel + x] = tile[q];
    }
}

}  // namespace vag
