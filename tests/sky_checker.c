/* CPU checker of Model.sky_image / Model.sky_moments (test infrastructure, not part of the engine).
 *
 * Follows the definition in INTEGRATION.md ("Sky images") literally on top of the plain-C oracle: run_pipeline, observe's EAT grids,
 * and for every (phi, theta) row and requested (nu, t) the very term specific_flux adds -- same bracket, same window, same
 * non-finite-slope rule, same normalisation --, placed on the sky and split over the row's azimuthal bin.  Compiled with the oracle's
 * flags (-std=c11 -O2 -ffp-contract=off) by tests/_skycheck.py for the sky-image tests. */
#include "../oracle/vag_oracle.c"

typedef struct {
    int g; /* l * nt + idx */
    double w, X, Y;
} sky_pt;

typedef struct {
    sky_pt* p;
    size_t n, cap;
} sky_list;

static void sky_push(sky_list* L, int g, double w, double X, double Y) {
    if (L->n == L->cap) {
        L->cap = L->cap ? 2 * L->cap : 4096;
        L->p = realloc(L->p, L->cap * sizeof(sky_pt));
    }
    L->p[L->n].g = g, L->p[L->n].w = w, L->p[L->n].X = X, L->p[L->n].Y = Y;
    L->n++;
}

/* the terms of one emitter pass (specific_flux's loops) -> splat points */
static void sky_terms(const pipeline_t* pl, const shock_t* sh, cell_eval_fn eval, void* grid, const double* t_obs, int nt_obs,
                      const double* nu_obs, int nnu, int n_az, sky_list* L) {
    const eat_t* o = &pl->eat;
    const coord_t* c = &pl->coord;
    const int t_grid = o->n_t;
    const double norm = o->one_plus_z / (o->lumi_dist * o->lumi_dist) / U_FLUX_DEN_CGS;
    const double D_A = o->lumi_dist / (o->one_plus_z * o->one_plus_z);
    const double sin_v = sin(c->theta_view), cos_v = cos(c->theta_view);
    double* lg2_t_obs = malloc(sizeof(double) * nt_obs);
    double* lg2_nu_src = malloc(sizeof(double) * nnu);
    for (int i = 0; i < nt_obs; ++i) lg2_t_obs[i] = log2(t_obs[i]);
    for (int l = 0; l < nnu; ++l) lg2_nu_src[l] = log2(nu_obs[l]) + log2(o->one_plus_z);
    const int npe = o->n_phi_eff, last_phi = npe - 1;
    for (int i = 0; i < npe; ++i) {
        /* the azimuthal bin of phi node i */
        double left, width;
        int mirrored = 0;
        if (npe == 1) {
            left = 0.0, width = 2 * C_PI;
        } else if (c->phi_mirrored) {
            mirrored = 1;
            left = (i > 0) ? 0.5 * (c->phi[i - 1] + c->phi[i]) : 0.0;
            width = ((i < last_phi) ? 0.5 * (c->phi[i] + c->phi[i + 1]) : C_PI) - left;
        } else {
            left = (i > 0) ? 0.5 * (c->phi[i - 1] + c->phi[i]) : c->phi[0];
            width = ((i < last_phi) ? 0.5 * (c->phi[i] + c->phi[i + 1]) : c->phi[last_phi]) - left;
        }
        int S = (int)ceil((double)n_az * width / (2 * C_PI));
        if (S < 1) S = 1;
        for (int j = 0; j < o->n_theta; ++j) {
            const size_t row = ((size_t)i * o->n_theta + j) * t_grid;
            const int cell_row = (o->phi_size > 1 ? i : 0) * o->n_theta + j;
            const double* t_row = o->lg2_t + row;
            const double* dop_row = o->lg2_doppler + row;
            const double* geom_row = o->lg2_geom + row;
            int k_lo, k_hi;
            if (!observed_window(t_row, t_grid, lg2_t_obs[0], lg2_t_obs[nt_obs - 1], &k_lo, &k_hi)) continue;
            for (int idx = 0; idx < nt_obs; ++idx) {
                const double tq = lg2_t_obs[idx];
                int k = -1;
                for (int kk = k_lo; kk < k_hi; ++kk)
                    if (t_row[kk] <= tq && tq < t_row[kk + 1]) k = kk;
                if (k < 0) continue;
                const double inv_t_ratio = 1.0 / (t_row[k + 1] - t_row[k]);
                const double f = (tq - t_row[k]) * inv_t_ratio;
                const size_t s0 = (size_t)cell_row * t_grid + k, s1 = s0 + 1;
                const double r = exp2(log2(sh->r[s0]) + f * (log2(sh->r[s1]) - log2(sh->r[s0])));
                const double th = c->spreading ? sh->theta[s0] + f * (sh->theta[s1] - sh->theta[s0]) : sh->theta[(size_t)cell_row * t_grid];
                for (int l = 0; l < nnu; ++l) {
                    const double b0 = eval(grid, cell_row, k, t_grid, lg2_nu_src[l] - dop_row[k]) + geom_row[k];
                    const double b1 = eval(grid, cell_row, k + 1, t_grid, lg2_nu_src[l] - dop_row[k + 1]) + geom_row[k + 1];
                    const double slope = (b1 - b0) * inv_t_ratio;
                    if (!isfinite(slope)) continue;
                    const double w = exp2(b0 + (tq - t_row[k]) * slope) * norm;
                    if (!(w > 0)) continue;
                    const double part = w / S;
                    for (int q = 0; q < S; ++q) {
                        const double ph = left + (q + 0.5) * (width / S);
                        const double X = r * (cos(th) * sin_v - sin(th) * cos(ph) * cos_v) / D_A;
                        const double Y = r * sin(th) * sin(ph) / D_A;
                        if (mirrored) {
                            sky_push(L, l * nt_obs + idx, 0.5 * part, X, Y);
                            sky_push(L, l * nt_obs + idx, 0.5 * part, X, -Y);
                        } else {
                            sky_push(L, l * nt_obs + idx, part, X, Y);
                        }
                    }
                }
            }
        }
    }
    free(lg2_t_obs);
    free(lg2_nu_src);
}

/* the whole splat of a (t, nu) request: every enabled component, forward shock first */
static int sky_splat(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, int n_az, sky_list* L) {
    if (check_times(t, nt) != 0) return -1;
    if (nnu <= 0) return fail("frequency array must be non-empty");
    double* t_obs = malloc(sizeof(double) * nt);
    double* nu_obs = malloc(sizeof(double) * nnu);
    for (int i = 0; i < nt; ++i) t_obs[i] = t[i] * U_SEC;
    for (int l = 0; l < nnu; ++l) nu_obs[l] = nu[l] * U_HZ;
    double lo, hi;
    minmax(t_obs, nt, &lo, &hi);
    pipeline_t pl;
    int rc = run_pipeline(&pl, p, lo, hi);
    if (rc == 0) {
        emitter_t em[2];
        const int n_em = pipeline_emitters(&pl, p, em);
        for (int e = 0; e < n_em; ++e) {
            const shock_t* sh = e == 0 ? &pl.shock : &pl.rvs_shock;
            sky_terms(&pl, sh, eval_syn_cell, em[e].ph, t_obs, nt, nu_obs, nnu, n_az, L);
            if (em[e].ssc) {
                const size_t ncell = (size_t)pl.coord.phi_size * pl.coord.n_theta * pl.coord.n_t;
                icphoton_t* ic = make_ic_photons(&pl, &em[e], nu_obs, nnu);
                sky_terms(&pl, sh, eval_ic_cell, ic, t_obs, nt, nu_obs, nnu, n_az, L);
                free_ic_photons(ic, ncell);
            }
        }
        pipeline_free(&pl);
    }
    free(t_obs);
    free(nu_obs);
    return rc;
}

/* image [nnu][nt][npixel][npixel] ([iy][ix]), outside [nnu][nt] */
int sky_checker_image(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, double fov, int npixel, int n_az,
                      double* image, double* outside) {
    sky_list L = {NULL, 0, 0};
    const int rc = sky_splat(p, t, nt, nu, nnu, n_az, &L);
    if (rc == 0) {
        const size_t np2 = (size_t)npixel * npixel;
        memset(image, 0, sizeof(double) * np2 * nnu * nt);
        memset(outside, 0, sizeof(double) * nnu * nt);
        const double half = 0.5 * fov, delta = fov / npixel;
        for (size_t q = 0; q < L.n; ++q) {
            const sky_pt* s = &L.p[q];
            const double fx = floor((s->X + half) / delta), fy = floor((s->Y + half) / delta);
            if (fx >= 0 && fx < npixel && fy >= 0 && fy < npixel)
                image[(size_t)s->g * np2 + (size_t)fy * npixel + (size_t)fx] += s->w;
            else
                outside[s->g] += s->w;
        }
    }
    free(L.p);
    return rc;
}

/* moments [nnu][nt][6]: F, Xbar, Ybar, varX, varY, covXY (two passes) */
int sky_checker_moments(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, int n_az, double* moments) {
    sky_list L = {NULL, 0, 0};
    const int rc = sky_splat(p, t, nt, nu, nnu, n_az, &L);
    if (rc == 0) {
        const int n = nnu * nt;
        memset(moments, 0, sizeof(double) * 6 * n);
        for (size_t q = 0; q < L.n; ++q) {
            double* m = moments + 6 * L.p[q].g;
            m[0] += L.p[q].w, m[1] += L.p[q].w * L.p[q].X, m[2] += L.p[q].w * L.p[q].Y;
        }
        for (int g = 0; g < n; ++g) moments[6 * g + 1] /= moments[6 * g], moments[6 * g + 2] /= moments[6 * g];
        for (size_t q = 0; q < L.n; ++q) {
            double* m = moments + 6 * L.p[q].g;
            const double dx = L.p[q].X - m[1], dy = L.p[q].Y - m[2];
            m[3] += L.p[q].w * dx * dx, m[4] += L.p[q].w * dy * dy, m[5] += L.p[q].w * dx * dy;
        }
        for (int g = 0; g < n; ++g) {
            double* m = moments + 6 * g;
            if (m[0] > 0)
                m[3] /= m[0], m[4] /= m[0], m[5] /= m[0];
            else
                m[1] = m[2] = m[3] = m[4] = m[5] = NAN;
        }
    }
    free(L.p);
    return rc;
}
