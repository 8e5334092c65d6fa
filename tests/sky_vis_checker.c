/* CPU checker of Model.sky_visibilities (test infrastructure, not part of the engine).
 *
 * The parts of sky_checker.c's splat ("Sky images"), placed on the sky with the position angle and summed as a direct
 * Fourier sum: V(u, v) = sum w exp(-2 pi i (u east + v north)), east = X sin pa + Y cos pa, north = X cos pa - Y sin pa.  The phase in
 * turns is reduced exactly (fmod) before it meets pi.  Compiled with the oracle's flags by tests/_vischeck.py. */
#include "sky_checker.c"

/* sin(pi x), cos(pi x) with x reduced exactly to [-1, 1] */
static void sincos_pi(double x, double* s, double* c) {
    double r = fmod(x, 2.0);
    if (r > 1.0) r -= 2.0;
    if (r < -1.0) r += 2.0;
    *s = sin(C_PI * r);
    *c = cos(C_PI * r);
}

/* u, v [nnu][nt][nbl] wavelengths; vis [nnu][nt][nbl][2] (re, im) */
int sky_checker_visibility(const vag_model_params* p, const double* t, int nt, const double* nu, int nnu, const double* u,
                           const double* v, int nbl, double pa, int n_az, double* vis) {
    sky_list L = {NULL, 0, 0};
    const int rc = sky_splat(p, t, nt, nu, nnu, n_az, &L);
    if (rc == 0) {
        const double sp = sin(pa), cp = cos(pa);
        memset(vis, 0, sizeof(double) * 2 * (size_t)nnu * nt * nbl);
        for (size_t q = 0; q < L.n; ++q) {
            const sky_pt* s = &L.p[q];
            const double east = s->X * sp + s->Y * cp, north = s->X * cp - s->Y * sp;
            const double* ug = u + (size_t)s->g * nbl;
            const double* vg = v + (size_t)s->g * nbl;
            double* o = vis + (size_t)s->g * nbl * 2;
            for (int k = 0; k < nbl; ++k) {
                double sn, cs;
                sincos_pi(2 * (ug[k] * east + vg[k] * north), &sn, &cs);
                o[2 * k] += s->w * cs;
                o[2 * k + 1] -= s->w * sn;
            }
        }
    }
    free(L.p);
    return rc;
}
