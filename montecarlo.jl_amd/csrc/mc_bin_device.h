// mc_bin_device.h — a section of the classical MC flavor's logarithmic binner as the measurement kernels behind a sweep
// see it (ising_fss.inl, qs_scaling.inl, qs_stiffness.inl), and the push of a section whose pairs share their first
// element.  The host side of a section is mc_bin_section (mc_host.h), which fills the argument.  The main sections, pushed
// inside the sweep kernels from registers (ising_bin_push, qs_bin_push), have their own fixed-size forms.
#pragma once

#include <hip/hip_runtime.h>

// kernel argument: the state of one section, [L][n_elem][W] for xs and x2, [L][n_pairs][W] for xy, [L - 1][n_comp][W]
// for the compressor c.  xs == nullptr: the section is off.  The last six fields of the struct that holds it.
struct mc_bin_arg {
    double *xs, *x2, *xy, *c;
    int lmax, top;  // trailing 1-bits of the push count (capped at top), the last level
};

// The push of pair k with the values (a, b) of a section with ne elements and np pairs in which pair k = (element 0,
// element 1 + k), state [level][element][walker].  lmax is the same in every lane: the levels below it complete a pair
// with their compressor and carry the average upwards, level lmax keeps the value.  The pairs of a walker are pushed by
// different lanes or workgroups and share nothing they write: each has its own element, its own cross sum and - so that
// none reads what another one writes - its own copy of element 0's compressor, [level][pair][2][walker] (the copies hold
// the same values; pair 0 alone adds element 0 to x_sum and x2_sum).
__device__ __forceinline__ void mc_bin_push_shared(const mc_bin_arg &f, size_t ne, size_t np, int W, int w, int k, double a,
                                                   double b)
{
    const size_t sW = (size_t)W;
    size_t ie = (size_t)(1 + k) * sW + w, i0 = (size_t)w, ip = (size_t)k * sW + w, ic = (size_t)k * 2 * sW + w;
    for (int l = 0;; ++l, ie += ne * sW, i0 += ne * sW, ip += np * sW, ic += 2 * np * sW) {
        const bool last = l == f.lmax;
        const double s1 = f.xs[ie], s2 = f.x2[ie], p = f.xy[ip];  // a level's values are requested together
        double ca = 0.0, cb = 0.0, t1 = 0.0, t2 = 0.0;
        if (!last) {
            ca = f.c[ic];
            cb = f.c[ic + sW];
        }
        if (k == 0) {
            t1 = f.xs[i0];
            t2 = f.x2[i0];
        }
        f.xs[ie] = s1 + b;
        f.x2[ie] = s2 + b * b;
        f.xy[ip] = p + a * b;
        if (k == 0) {
            f.xs[i0] = t1 + a;
            f.x2[i0] = t2 + a * a;
        }
        if (last) break;
        a = 0.5 * (ca + a);
        b = 0.5 * (cb + b);
    }
    if (f.lmax < f.top) {  // (the top level has no compressor)
        f.c[ic] = a;
        f.c[ic + sW] = b;
    }
}
