// Acquisition formulas as device functions, shared by the batched kernels (grad.hip) and the fused one-row path (onerow.hip).
// Reference: GPyOpt/GPyOpt/util/general.py:113-129 (get_quantiles), acquisitions/EI.py:32-51, LCB.py:31-46, MPI.py:32-51,
// models/gpmodel.py:95-142 (clip at 1e-10, dsdx = dvdx / (2 sqrt(v))), acquisitions/LP.py:40-140.
#pragma once
#include "gphip_internal.h"
#include "../../include/gphip.h"

// Value f and the two partial derivatives of one acquisition at (mean, var) of the NORMALISED model:
//   d f / dx = c_m * (y_std * dmdx) + c_s * (ds_scale * dvdx)
// (un-normalisation gp.py:344-352; clip gpmodel.py:99; s floor general.py:121-124).
__device__ __forceinline__ void acq_terms(int type, double par, double fmin, double y_mean, double y_std, double mean,
                                          double var, double &f, double &c_m, double &c_s, double &ds_scale) {
    const double m = mean * y_std + y_mean;
    double v = var * (y_std * y_std);
    v = (v < 1e-10) ? 1e-10 : v;
    double s = sqrt(v);
    ds_scale = (y_std * y_std) / (2.0 * s);  // dsdx = dvdx / (2 sqrt(v)), gpmodel.py:140
    if (type == GP_ACQ_LCB) {
        f = -m + par * s;
        c_m = -1.0;
        c_s = par;
    } else {
        if (s < 1e-10) s = 1e-10;
        const double u = (fmin - m - par) / s;
        const double phi = exp(-0.5 * u * u) / 2.50662827463100050241576528481105;
        const double Phi = 0.5 * erfc(-u / 1.41421356237309504880168872420970);
        if (type == GP_ACQ_EI) {
            f = s * (u * Phi + phi);
            c_m = -Phi;
            c_s = phi;
        } else {
            f = Phi;
            c_m = -(phi / s);
            c_s = -(phi / s) * u;
        }
    }
}

// scipy.stats.norm.logcdf == cephes log_ndtr: log(ndtr(z)) for z > -20, the asymptotic series below it, -ndtr(-z) above 6.
__device__ __forceinline__ double gp_log_ndtr(double z) {
    if (z > 6.0) return -0.5 * erfc(z / 1.41421356237309504880168872420970);
    if (z > -20.0) return log(0.5 * erfc(-z / 1.41421356237309504880168872420970));
    const double log_lhs = -0.5 * z * z - log(-z) - 0.5 * log(2.0 * 3.14159265358979323846);
    double last_total = 0.0, right_hand_side = 1.0, numerator = 1.0, denom_factor = 1.0;
    const double denom_cons = 1.0 / (z * z);
    long sign = 1, i = 0;
    while (fabs(last_total - right_hand_side) > 2.220446049250313e-16) {
        i += 1;
        last_total = right_hand_side;
        sign = -sign;
        denom_factor *= denom_cons;
        numerator *= (double)(2 * i - 1);
        right_hand_side += (double)sign * numerator * denom_factor;
        if (i > 200) break;
    }
    return log_lhs + log(right_hand_side);
}

// One black-box constraint's share of the probability of feasibility at a location (Gardner et al. 2014; Gelbart et al. 2014):
// (mean, var) of the constraint GP's NORMALISED posterior, (c_mean, c_std) its output normaliser, b its upper bound.  Un-normalised
// and clipped exactly as acq_terms does; z = (b - m) / s.  Out: log Phi(z), and what feas_grad needs -- the inverse Mills ratio
// lambda(z) = phi(z) / Phi(z) = exp(-z^2 / 2 - log(2 pi) / 2 - log Phi(z)), formed in log space: it stays finite (~ -z) where Phi
// underflows, and nothing is divided by a Phi that rounded to zero.
__device__ __forceinline__ void feas_terms(double mean, double var, double c_mean, double c_std, double b, double &logphi,
                                           double &lam, double &z, double &s) {
    const double m = mean * c_std + c_mean;
    double v = var * (c_std * c_std);
    v = (v < 1e-10) ? 1e-10 : v;
    s = sqrt(v);
    z = (b - m) / s;
    logphi = gp_log_ndtr(z);
    lam = exp(-0.5 * z * z - 0.91893853320467274178032973640562 - logphi);
}
// d log Phi(z) / dx_d = lambda (-dm - z ds) / s with dm = c_std dmdx, ds = c_std^2 dvdx / (2 s)
__device__ __forceinline__ double feas_grad(double lam, double z, double s, double c_std, double dmdx, double dvdx) {
    const double dm = c_std * dmdx;
    const double ds = (c_std * c_std) * dvdx / (2.0 * s);
    return lam * (-dm - z * ds) / s;
}

// ---- expected hypervolume improvement (Emmerich et al. 2011; Yang et al. 2019) ---------------------------------------------------
// One coordinate c of the cell decomposition against one objective at a location: (mean, var) of the objective GP's NORMALISED
// posterior, (y_mean, y_std) its output normaliser, un-normalised and clipped exactly as acq_terms does.  z = (c - m) / s,
//   Psi = s (z Phi(z) + phi(z))   -- EI with incumbent c and no jitter: d Psi / dm = -Phi, d Psi / ds = phi --
// and c = -inf (index 0 of every level array) yields zeros.  No product is contracted into an fma: the bits are those of the
// operations as written, whatever the surrounding kernel.
__device__ __forceinline__ void ehvi_level(double mean, double var, double y_mean, double y_std, double c, double &Psi, double &Phi,
                                           double &phi, double &s) {
#pragma clang fp contract(off)
    const double m = mean * y_std + y_mean;
    double v = var * (y_std * y_std);
    v = (v < 1e-10) ? 1e-10 : v;
    s = sqrt(v);
    if (c == -INFINITY) {
        Psi = Phi = phi = 0.0;
        return;
    }
    const double z = (c - m) / s;
    phi = exp(-0.5 * z * z) / 2.50662827463100050241576528481105;
    Phi = 0.5 * erfc(-z / 1.41421356237309504880168872420970);
    Psi = s * (z * Phi + phi);
}

// ---- max-value entropy search (Wang & Jegelka, ICML 2017), mirrored for a minimum ------------------------------------------------
// h(g) = g lambda(g) / 2 - log Phi(g) and h'(g) = -(lambda / 2) B(g), B = 1 + g^2 + g lambda, lambda = phi / Phi.
// g > -20: log Phi by gp_log_ndtr, lambda = exp(-g^2 / 2 - log(2 pi) / 2 - log Phi) in log space as feas_terms forms it, h and B
// from their terms.
// g <= -20 -- where gp_log_ndtr switches to the asymptotic series as well -- those forms cancel: B -> 2 / g^2 loses g^4 / 2 ulp, h
// ~ log|g| is the difference of two terms of size g^2 / 2, and so is lambda's exponent.  There everything comes from the series
// itself: with t = 1 / g^2, T_i = (-1)^i (2i - 1)!! t^i, R = 1 + sum_i T_i  (Phi(g) = phi(g) / (-g) R),
//     lambda = -g / R,   B = (sum_{i >= 1} -2 i T_i) / R = 2 t - 10 t^2 + 74 t^3 - ...,
//     h = W / (2 R) + log(-g) + log(2 pi) / 2 - log R,   W = sum_{i >= 1} T_i g^2 = -1 + 3 t - 15 t^2 + ...
// (g lambda / 2 = -g^2 / (2 R) and -log Phi = g^2 / 2 + log(-g) + log(2 pi) / 2 - log R: the two g^2 / 2 meet in (g^2 / 2)(R - 1) / R.)
// No term cancels at any g <= -20.  Sixteen terms: the first one dropped is below 1e-24 of the sums at g = -20 and falls with |g|.
__device__ __forceinline__ void mes_h(double g, double &h, double &hp) {
    if (g > -20.0) {
        const double logphi = gp_log_ndtr(g);
        const double lam = exp(-0.5 * g * g - 0.91893853320467274178032973640562 - logphi);
        h = 0.5 * g * lam - logphi;
        hp = -(0.5 * lam) * (1.0 + g * g + g * lam);
        return;
    }
    const double g2 = g * g, t = 1.0 / g2;
    double term = 1.0, R = 1.0, S = 0.0, W = 0.0;
    for (int i = 1; i <= 16; ++i) {
        term *= -(double)(2 * i - 1) * t;
        R += term;
        S += (double)(-2 * i) * term;
        W += term * g2;
    }
    const double lam = -g / R;
    h = W / (2.0 * R) + log(-g) + 0.91893853320467274178032973640562 - log(R);
    hp = -(0.5 * lam) * (S / R);
}

// MES at (mean, var) of the NORMALISED model over the K samples ystar [K] of the minimum's value (un-normalised, as fmin is):
//   g_k = (m - ystar_k) / s,  f = (1 / K) sum_k h(g_k)   (k = 0 .. K - 1 in index order)
//   c_m = d f / dm = ((1 / K) sum_k h'(g_k)) / s,  c_s = d f / ds = -((1 / K) sum_k h'(g_k) g_k) / s
// m, s and ds_scale exactly as acq_terms forms them.  h and h' stay finite where Phi underflows (g << 0) and go to 0 without
// leaving the finite range where phi does (g >> 0).
__device__ __forceinline__ void mes_terms(const double *ystar, int K, double y_mean, double y_std, double mean, double var, double &f,
                                          double &c_m, double &c_s, double &ds_scale) {
    const double m = mean * y_std + y_mean;
    double v = var * (y_std * y_std);
    v = (v < 1e-10) ? 1e-10 : v;
    const double s = sqrt(v);
    ds_scale = (y_std * y_std) / (2.0 * s);
    double sh = 0.0, sm = 0.0, ss = 0.0;
    for (int k = 0; k < K; ++k) {
        const double g = (m - ystar[k]) / s;
        double h, hp;
        mes_h(g, h, hp);
        sh += h;
        sm += hp;
        ss += hp * g;
    }
    f = sh / (double)K;
    c_m = (sm / (double)K) / s;
    c_s = -((ss / (double)K) / s);
}

// AcquisitionLP._penalized_acquisition (LP.py:70-89) for one location: negacq = -acq(x) in, the penalised score out.
// transform: 0 = none (log(acq + 1e-50)), 1 = softplus (LP.py:77-83)
__device__ __forceinline__ double lp_value(double negacq, const double *x, int D, const double *Xb, int nb, const double *r0,
                                           const double *s0, int transform) {
    double f = -negacq;
    if (transform == 1)
        f = (f >= 40.0) ? log(f) : log(log1p(exp(f)));
    else
        f = log(f + 1e-50);
    f = -f;
    for (int k = 0; k < nb; ++k) {
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double df = x[d] - Xb[k * D + d];
            d2 = fma(df, df, d2);
        }
        f -= gp_log_ndtr((sqrt(d2) - r0[k]) / s0[k]);
    }
    return f;
}

// Value and gradient of the penalised acquisition (LP.py:112-140): negacq = -acq(x) and dneg[D] = -d acq / dx in, overwritten
// by the penalised value's gradient; returns the penalised value.  The penaliser's gradient is the reference's: one scalar
// per (location, centre) summed over the batch and subtracted from every dimension (LP.py:91-103 has no direction factor).
__device__ __forceinline__ double lp_value_grad(double negacq, double *dneg, const double *x, int D, const double *Xb, int nb,
                                                const double *r0, const double *s0, int transform) {
    const double a = -negacq;
    double f, scale;
    if (transform == 1) {
        const double sp = log1p(exp(a));
        f = (a >= 40.0) ? log(a) : log(sp);
        scale = 1.0 / (sp * (1.0 + exp(-a)));
    } else {
        f = log(a + 1e-50);
        scale = 1.0 / a;
    }
    f = -f;
    double pen = 0.0;
    for (int k = 0; k < nb; ++k) {
        double d2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double df = x[d] - Xb[k * D + d];
            d2 = fma(df, df, d2);
        }
        const double nm = sqrt(d2);
        const double z = (nm - r0[k]) / s0[k];
        f -= gp_log_ndtr(z);
        const double cdf = 0.5 * erfc(-z / 1.41421356237309504880168872420970);
        if (!(cdf < 1e-50)) pen += 1.0 / (s0[k] * 2.50662827463100050241576528481105 * cdf) * exp(-0.5 * z * z) / nm;
    }
    for (int d = 0; d < D; ++d) dneg[d] = scale * dneg[d] - pen;
    return f;
}
