/* CPU checker of Model.sky_polarization / Model.sky_stokes_image (test infrastructure, not part of the engine).
 *
 * Follows the bullet "Polarization" of INTEGRATION.md ("Sky images") literally on top of the plain-C oracle: the parts of
 * sky_checker.c's splat -- same rows, brackets, weights and positions --, each with the Lorentz factor of its emitter's own shock_t
 * (Gamma beta interpolated in the f that interpolates lg2 r), the cosine mu between the line of sight and the radial direction, the
 * fluid-frame s = sin^2 theta', the local degree Pi of a random field of anisotropy b, and Q, U about the projected radial direction.
 * One emitter / pass flag per part: an SSC part is unpolarized.  Compiled with the oracle's flags by tests/_polcheck.py. */
#include "sky_checker.c"

typedef struct {
    double b[2], pi_max[2]; /* vag_pol_spec: 0 forward, 1 reverse shock; pi_max < 0: (p + 1) / (p + 7/3) */
} pol_spec;

typedef struct {
    int g;        /* l * nt + idx */
    int mirrored; /* one half (at +Y or -Y) of a part of a mirrored grid */
    double w, X, Y, Pi;
} pol_pt;

typedef struct {
    pol_pt* p;
    size_t n, cap;
} pol_list;

static void pol_push(pol_list* L, int g, int mirrored, double w, double X, double Y, double Pi) {
    if (L->n == L->cap) {
        L->cap = L->cap ? 2 * L->cap : 4096;
        L->p = realloc(L->p, L->cap * sizeof(pol_pt));
    }
    pol_pt* q = &L->p[L->n++];
    q->g = g, q->mirrored = mirrored, q->w = w, q->X = X, q->Y = Y, q->Pi = Pi;
}

/* sky_terms (sky_checker.c) with the polarization of every part; polarized = 0: an SSC pass */
static void pol_terms(const pipeline_t* pl, const shock_t* sh, cell_eval_fn eval, void* grid, const double* t_obs, int nt_obs,
                      const double* nu_obs, int nnu, int n_az, int polarized, double b, double pi_max, pol_list* L) {
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
                const double u0 = sqrt((sh->Gamma[s0] - 1) * (sh->Gamma[s0] + 1)), u1 = sqrt((sh->Gamma[s1] - 1) * (sh->Gamma[s1] + 1));
                const double u = u0 + f * (u1 - u0);
                const double Gam = sqrt(1 + u * u);
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
                        double Pi = 0.0;
                        if (polarized) {
                            const double mu = cos(th) * cos_v + sin(th) * sin_v * cos(ph);
                            double s = (1 - mu * mu) / ((Gam - u * mu) * (Gam - u * mu));
                            s = s < 0 ? 0 : (s > 1 ? 1 : s);
                            Pi = pi_max * ((b - 1) * s / (2 + (b - 1) * s));
                        }
                        if (mirrored) {
                            pol_push(L, l * nt_obs + idx, 1, 0.5 * part, X, Y, Pi);
                            pol_push(L, l * nt_obs + idx, 1, 0.5 * part, X, -Y, Pi);
                        } else {
                            pol_push(L, l * nt_obs + idx, 0, part, X, Y, Pi);
                        }
                    }
                }
            }
        }
    }
    free(lg2_t_obs);
    free(lg2_nu_src);
}

/* sky_splat with the polarization spec */
static int pol_splat(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, const pol_spec* pol, int n_az,
                     pol_list* L) {
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
            const double pe = e == 0 ? p->p : p->rvs_p;
            const double pi_max = pol->pi_max[e] < 0 ? (pe + 1) / (pe + 7.0 / 3.0) : pol->pi_max[e];
            pol_terms(&pl, sh, eval_syn_cell, em[e].ph, t_obs, nt, nu_obs, nnu, n_az, 1, pol->b[e], pi_max, L);
            if (em[e].ssc) {
                const size_t ncell = (size_t)pl.coord.phi_size * pl.coord.n_theta * pl.coord.n_t;
                icphoton_t* ic = make_ic_photons(&pl, &em[e], nu_obs, nnu);
                pol_terms(&pl, sh, eval_ic_cell, ic, t_obs, nt, nu_obs, nnu, n_az, 0, 1.0, 0.0, L);
                free_ic_photons(ic, ncell);
            }
        }
        pipeline_free(&pl);
    }
    free(t_obs);
    free(nu_obs);
    return rc;
}

/* Q and U of one point about the projected radial direction psi = atan2(Y, X) */
static void pol_qu(const pol_pt* s, double* q, double* u) {
    const double r2 = s->X * s->X + s->Y * s->Y;
    *q = 0.0, *u = 0.0;
    if (r2 > 0) {
        *q = -s->Pi * s->w * (s->X * s->X - s->Y * s->Y) / r2;
        *u = -s->Pi * s->w * 2 * s->X * s->Y / r2;
    }
}

/* out [nnu][nt][3]: I, Q, U on the sky, +X at position angle pa east of north */
int sky_checker_polarization(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, const pol_spec* pol,
                             double pa, int n_az, double* out) {
    pol_list L = {NULL, 0, 0};
    const int rc = pol_splat(p, t, nt, nu, nnu, pol, n_az, &L);
    if (rc == 0) {
        const int n = nnu * nt;
        memset(out, 0, sizeof(double) * 3 * n);
        for (size_t k = 0; k < L.n; ++k) {
            const pol_pt* s = &L.p[k];
            double q, u;
            pol_qu(s, &q, &u);
            double* o = out + 3 * s->g;
            o[0] += s->w;
            o[1] += q;
            if (!s->mirrored) o[2] += u; /* the halves of a mirrored part: +u and -u, nothing to U */
        }
        const double c2 = cos(2 * pa), s2 = sin(2 * pa);
        for (int g = 0; g < n; ++g) {
            const double Q = out[3 * g + 1], U = out[3 * g + 2];
            out[3 * g + 1] = Q * c2 - U * s2;
            out[3 * g + 2] = Q * s2 + U * c2;
        }
    }
    free(L.p);
    return rc;
}

/* image [nnu][nt][3][npixel][npixel] ([iy][ix]) in the jet frame, outside [nnu][nt][3] */
int sky_checker_stokes_image(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, const pol_spec* pol,
                             double fov, int npixel, int n_az, double* image, double* outside) {
    pol_list L = {NULL, 0, 0};
    const int rc = pol_splat(p, t, nt, nu, nnu, pol, n_az, &L);
    if (rc == 0) {
        const size_t np2 = (size_t)npixel * npixel;
        memset(image, 0, sizeof(double) * 3 * np2 * nnu * nt);
        memset(outside, 0, sizeof(double) * 3 * nnu * nt);
        const double half = 0.5 * fov, delta = fov / npixel;
        for (size_t k = 0; k < L.n; ++k) {
            const pol_pt* s = &L.p[k];
            double v[3];
            v[0] = s->w;
            pol_qu(s, &v[1], &v[2]);
            const double fx = floor((s->X + half) / delta), fy = floor((s->Y + half) / delta);
            const int in = fx >= 0 && fx < npixel && fy >= 0 && fy < npixel;
            for (int q = 0; q < 3; ++q) {
                if (in)
                    image[((size_t)s->g * 3 + q) * np2 + (size_t)fy * npixel + (size_t)fx] += v[q];
                else
                    outside[3 * s->g + q] += v[q];
            }
        }
    }
    free(L.p);
    return rc;
}
