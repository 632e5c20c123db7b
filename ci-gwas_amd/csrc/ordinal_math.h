// ordinal_math.h -- the arithmetic of the polychoric / polyserial estimators (cusk_polychoric_fit, cusk_polyserial_fit of
// include/cusk_hip.h), in IEEE double, written once for the device kernels of ordinal.hip and for the host self test
// (tools/ordinal_selftest.cpp), which compiles the same text with a C++ compiler.
//
//   Phi2     standard bivariate normal distribution function by Genz's algorithm (A. Genz, "Numerical computation of
//            rectangular bivariate and trivariate normal and t probabilities", Statistics and Computing 14 (2004): the
//            Drezner-Wesolowsky integral over asin(rho) with 6 / 12 / 20 Gauss-Legendre points, and the expansion
//            around |rho| = 1 from 0.925 on), written out from the published method
//   qnorm    Wichura's AS 241 (PPND16) with one Newton step on erfc, the form of thresholds.cpp
//   RootIter the safeguarded Newton iteration on a score: both estimators solve l'(rho) = 0 on [-0.9999, 0.9999] from
//            the score and its derivative, and fall back to bisection of the bracket when a step leaves it
//
// The two-step estimators hold the thresholds fixed, so a likelihood is a function of rho alone.  A cell (or an
// observation) whose probability underflows where it has observations makes the likelihood -infinity there; at rho = 0
// every such probability is a product of positive shares, so the maximum lies on the zero side of such a point and the
// iteration is told so (`barrier`) instead of being handed a quotient of two underflows.  "Underflows" means below 1e-14:
// a rectangle probability is a difference of four distribution values, each good to about 1e-16.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ORD_HD __host__ __device__ __forceinline__
#else
#define ORD_HD inline
#endif

namespace cusk {
namespace ord {

constexpr double kRhoMax = 0.9999;
constexpr double kTinyProb = 1e-14;  // below this a probability is rounding noise of the distribution values it is a difference of
constexpr int kStatusOk = 0, kStatusBoundary = 1, kStatusDegenerate = 2;
constexpr int kMaxLevels = 8;

ORD_HD double phi(double x) { return 0.3989422804014326779 * exp(-0.5 * x * x); }
ORD_HD double Phi(double x) { return 0.5 * erfc(-x * 0.70710678118654752440); }

ORD_HD double ppnd16(double p)
{
    const double q = p - 0.5;
    double r, val;
    if (fabs(q) <= 0.425)
    {
        r = 0.180625 - q * q;
        return q *
               (((((((2.5090809287301226727e3 * r + 3.3430575583588128105e4) * r + 6.7265770927008700853e4) * r +
                    4.5921953931549871457e4) * r + 1.3731693765509461125e4) * r + 1.9715909503065514427e3) * r +
                 1.3314166789178437745e2) * r + 3.3871328727963666080e0) /
               (((((((5.2264952788528545610e3 * r + 2.8729085735721942674e4) * r + 3.9307895800092710610e4) * r +
                    2.1213794301586595867e4) * r + 5.3941960214247511077e3) * r + 6.8718700749205790830e2) * r +
                 4.2313330701600911252e1) * r + 1.0);
    }
    r = (q < 0.0) ? p : 1.0 - p;
    if (r <= 0.0) return (q < 0.0) ? -INFINITY : INFINITY;
    r = sqrt(-log(r));
    if (r <= 5.0)
    {
        r -= 1.6;
        val = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                   1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
                4.63033784615654529590e0) * r + 1.42343711074968357734e0) /
              (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                   1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
                2.05319162663775882187e0) * r + 1.0);
    }
    else
    {
        r -= 5.0;
        val = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                   2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
                5.46378491116411436990e0) * r + 6.65790464350110377720e0) /
              (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                   7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555887937690e-1) * r + 1.0);
    }
    return (q < 0.0) ? -val : val;
}

// the threshold below which `cum` of `n` observations lie: -inf / +inf at the ends
ORD_HD double threshold_of(long long cum, long long n)
{
    if (cum <= 0) return -INFINITY;
    if (cum >= n) return INFINITY;
    const double p = (double)cum / (double)n;
    double x = ppnd16(p);
    const double e = Phi(x) - p;
    x -= e * 2.50662827463100050242 * exp(0.5 * x * x);
    return x;
}

// Gauss-Legendre abscissae and weights on [-1, 1] (positive half; the rule is symmetric): 6 points at [0, 3), 12 at
// [3, 9), 20 at [9, 19).  One table read in a loop, in constant memory on the device: the three rules share their code.
#if defined(__HIP_DEVICE_COMPILE__)
#define ORD_TABLE static __device__ __constant__ const double
#else
#define ORD_TABLE static const double
#endif
ORD_TABLE kGLX[19] = {0.9324695142031522,  0.6612093864662647, 0.2386191860831970, 0.9815606342467191, 0.9041172563704750,
                      0.7699026741943050,  0.5873179542866171, 0.3678314989981802, 0.1252334085114692, 0.9931285991850949,
                      0.9639719272779138,  0.9122344282513259, 0.8391169718222188, 0.7463319064601508, 0.6360536807265150,
                      0.5108670019508271,  0.3737060887154196, 0.2277858511416451, 0.07652652113349733};
ORD_TABLE kGLW[19] = {0.1713244923791705,  0.3607615730481384,  0.4679139345726904,  0.04717533638651177, 0.1069393259953183,
                      0.1600783285433464,  0.2031674267230659,  0.2334925365383547,  0.2491470458134029,  0.01761400713915212,
                      0.04060142980038694, 0.06267204833410906, 0.08327674157670475, 0.1019301198172404,  0.1181945319615184,
                      0.1316886384491766,  0.1420961093183821,  0.1491729864726037,  0.1527533871307259};

// P(X > h, Y > k) at correlation r, finite h and k, |r| < 0.925: nodes [first, first + count) of the table
ORD_HD double bvu_mid(int first, int count, double h, double k, double r)
{
    const double hk = h * k, hs = 0.5 * (h * h + k * k), asr = 0.5 * asin(r);
    double sum = 0.0;
#pragma unroll 1
    for (int i = first; i < first + count; i++)
    {
        const double x = kGLX[i], w = kGLW[i];
        const double sn = sin(asr * (1.0 - x)), sp = sin(asr * (1.0 + x));
        sum += w * exp((sn * hk - hs) / (1.0 - sn * sn));
        sum += w * exp((sp * hk - hs) / (1.0 - sp * sp));
    }
    return sum * asr * 0.15915494309189533577 + Phi(-h) * Phi(-k);
}

ORD_HD double bvu(double h, double k, double r)
{
    const double ar = fabs(r);
    if (r == 0.0) return Phi(-h) * Phi(-k);
    double bvn;
    if (ar < 0.925)
        bvn = ar < 0.3 ? bvu_mid(0, 3, h, k, r) : ar < 0.75 ? bvu_mid(3, 6, h, k, r) : bvu_mid(9, 10, h, k, r);
    else
    {
        const double tp = 6.28318530717958647692;
        double hk = h * k;
        if (r < 0.0)
        {
            k = -k;
            hk = -hk;
        }
        bvn = 0.0;
        if (ar < 1.0)
        {
            const double as = 1.0 - r * r, bs = (h - k) * (h - k);
            double a = sqrt(as);
            const double c = (4.0 - hk) / 8.0, d = (12.0 - hk) / 80.0;
            const double asr0 = -0.5 * (bs / as + hk);
            if (asr0 > -100.0) bvn = a * exp(asr0) * (1.0 - c * (bs - as) * (1.0 - d * bs) / 3.0 + c * d * as * as);
            if (hk > -100.0)
            {
                const double b = sqrt(bs), sp = sqrt(tp) * Phi(-b / a);
                bvn -= exp(-0.5 * hk) * sp * b * (1.0 - c * bs * (1.0 - d * bs) / 3.0);
            }
            a *= 0.5;
            double sum = 0.0;
#pragma unroll 1
            for (int i = 0; i < 20; i++)
            {
                const double t = a * (i < 10 ? 1.0 - kGLX[9 + i] : 1.0 + kGLX[i - 1]), xs = t * t;
                const double asr = -0.5 * (bs / xs + hk);
                if (asr > -100.0)
                {
                    const double sp = 1.0 + c * xs * (1.0 + 5.0 * d * xs);
                    const double rs = sqrt(1.0 - xs);
                    const double ep = exp(-0.5 * hk * xs / ((1.0 + rs) * (1.0 + rs))) / rs;
                    sum += kGLW[i < 10 ? 9 + i : i - 1] * exp(asr) * (sp - ep);
                }
            }
            bvn = (a * sum - bvn) / tp;
        }
        if (r > 0.0)
            bvn += Phi(-fmax(h, k));
        else if (h >= k)
            bvn = -bvn;
        else
        {
            const double L = h < 0.0 ? Phi(k) - Phi(h) : Phi(-h) - Phi(-k);
            bvn = L - bvn;
        }
    }
    return fmax(0.0, fmin(1.0, bvn));
}

// Phi2(h, k; r) = P(X <= h, Y <= k); either argument may be infinite
ORD_HD double Phi2(double h, double k, double r)
{
    if (h == -INFINITY || k == -INFINITY) return 0.0;
    if (h == INFINITY) return k == INFINITY ? 1.0 : Phi(k);
    if (k == INFINITY) return Phi(h);
    return bvu(-h, -k, r);
}

// the bivariate density at a finite corner (0 at an infinite one) and its derivative in rho
ORD_HD void phi2_d(double h, double k, double r, double &dens, double &ddens)
{
    dens = ddens = 0.0;
    if (!(fabs(h) < INFINITY) || !(fabs(k) < INFINITY)) return;
    const double s = 1.0 - r * r, Q = h * h - 2.0 * r * h * k + k * k;
    dens = 0.15915494309189533577 / sqrt(s) * exp(-0.5 * Q / s);
    ddens = dens * (r / s + h * k / s - r * Q / (s * s));
}

// Safeguarded Newton on a decreasing-through-zero score.  Protocol: rho() is the point to evaluate next; feed the score
// and its derivative there (or barrier = true) to step(); done() ends it.  The first two points are the ends of the
// interval: a score that is not negative at +kRhoMax, or not positive at -kRhoMax, ends on that boundary.
struct RootIter
{
    double lo, hi, x, dx;
    int phase, it, status;
    ORD_HD void start()
    {
        lo = -kRhoMax;
        hi = kRhoMax;
        x = kRhoMax;
        dx = 1.0;
        phase = 0;
        it = 0;
        status = kStatusOk;
    }
    ORD_HD double rho() const { return x; }
    ORD_HD bool done() const { return phase == 3; }
    ORD_HD void step(double score, double dscore, bool barrier)
    {
        if (barrier && x == 0.0) barrier = false;  // products of positive shares: nothing underflows at zero
        if (barrier) score = x > 0.0 ? -INFINITY : INFINITY;
        if (phase == 0)
        {  // at +kRhoMax
            if (score >= 0.0)
            {
                status = kStatusBoundary;
                phase = 3;
                return;
            }
            x = -kRhoMax;
            phase = 1;
            return;
        }
        if (phase == 1)
        {  // at -kRhoMax
            if (score <= 0.0)
            {
                status = kStatusBoundary;
                phase = 3;
                return;
            }
            x = 0.0;
            phase = 2;
            return;
        }
        it++;
        if (score == 0.0 || it >= 100)
        {
            phase = 3;
            return;
        }
        if (score > 0.0)
            lo = x;
        else
            hi = x;
        double nx = x - score / dscore;
        if (barrier || !(dscore < 0.0) || !(nx > lo && nx < hi)) nx = 0.5 * (lo + hi);
        dx = fabs(nx - x);
        x = nx;
        // Newton converges quadratically: a step below 1e-10 leaves an error below rounding; the rounding of the score
        // itself moves a step by more than 1e-13 at half a million observations, so nothing tighter would ever be met
        if (dx < 1e-10 || hi - lo < 1e-13) phase = 4;
    }
    // phase 4: one last evaluation at the final point gives the derivative the standard error is formed from
    ORD_HD bool last() const { return phase == 4; }
    ORD_HD void finish() { phase = 3; }
};

// r, se, status from the end of an iteration; d2 = l''(rho) at the final point
ORD_HD void conclude(const RootIter &it, double d2, double &r, double &se, int &status)
{
    r = it.x;
    status = it.status;
    se = NAN;
    if (status == kStatusOk)
    {
        if (-d2 > 0.0)
            se = 1.0 / sqrt(-d2);
        else
            status = kStatusBoundary;
    }
}

// The polychoric likelihood of one ka x kb table at rho: score, its derivative, barrier.  `cell(a, b)` returns n_ab;
// alpha[a * as] / beta[b * bs] are the upper thresholds of row a / column b (the last one +inf).  Walking a row, the two
// corners on the left of a cell are those on the right of the cell before it.
template <class Cell>
ORD_HD void polychoric_eval(const Cell &cell, int ka, int kb, const double *alpha, int as, const double *beta, int bs, double rho,
                            double &score, double &dscore, bool &barrier)
{
    score = dscore = 0.0;
    barrier = false;
    double a_lo = -INFINITY;
    for (int a = 0; a < ka; a++)
    {
        const double a_hi = alpha[a * as];
        double F_ll = 0.0, f_ll = 0.0, g_ll = 0.0, F_hl = 0.0, f_hl = 0.0, g_hl = 0.0;  // corners at beta = -inf
        for (int b = 0; b < kb; b++)
        {
            const double b_hi = beta[b * bs];
            double F_lh = 0.0, f_lh = 0.0, g_lh = 0.0, F_hh = 0.0, f_hh = 0.0, g_hh = 0.0;
#pragma unroll 1
            for (int side = 0; side < 2; side++)
            {  // the lower, then the upper corner on the right of the cell: one copy of the code
                const double av = side ? a_hi : a_lo;
                double f, g;
                const double F = Phi2(av, b_hi, rho);
                phi2_d(av, b_hi, rho, f, g);
                if (side)
                    F_hh = F, f_hh = f, g_hh = g;
                else
                    F_lh = F, f_lh = f, g_lh = g;
            }
            const int n = cell(a, b);
            if (n > 0)
            {
                const double pi = F_hh - F_lh - F_hl + F_ll;
                if (!(pi >= kTinyProb))
                    barrier = true;
                else
                {
                    const double d1 = (f_hh - f_lh - f_hl + f_ll) / pi, d2 = (g_hh - g_lh - g_hl + g_ll) / pi;
                    score += n * d1;
                    dscore += n * (d2 - d1 * d1);
                }
            }
            F_ll = F_lh, f_ll = f_lh, g_ll = g_lh;
            F_hl = F_hh, f_hl = f_hh, g_hl = g_hh;
        }
        a_lo = a_hi;
    }
}

// The whole polychoric fit of one table.  alpha / beta: scratch for ka / kb thresholds at strides as / bs.
template <class Cell>
ORD_HD void polychoric_fit(const Cell &cell, int ka, int kb, double *alpha, int as, double *beta, int bs, double &r, double &se,
                           int &status)
{
    long long n = 0;
    int rows_seen = 0, cols_seen = 0;
    for (int a = 0; a < ka; a++)
    {
        long long m = 0;
        for (int b = 0; b < kb; b++) m += cell(a, b);
        n += m;
        rows_seen += m > 0;
    }
    for (int b = 0; b < kb; b++)
    {
        long long m = 0;
        for (int a = 0; a < ka; a++) m += cell(a, b);
        cols_seen += m > 0;
    }
    if (rows_seen < 2 || cols_seen < 2)
    {
        r = se = NAN;
        status = kStatusDegenerate;
        return;
    }
    long long cum = 0;
    for (int a = 0; a < ka; a++)
    {
        for (int b = 0; b < kb; b++) cum += cell(a, b);
        alpha[a * as] = threshold_of(cum, n);
    }
    cum = 0;
    for (int b = 0; b < kb; b++)
    {
        for (int a = 0; a < ka; a++) cum += cell(a, b);
        beta[b * bs] = threshold_of(cum, n);
    }
    RootIter it;
    it.start();
    double d2 = 0.0;
    while (!it.done())
    {
        double sc, dsc;
        bool barrier;
        polychoric_eval(cell, ka, kb, alpha, as, beta, bs, it.rho(), sc, dsc, barrier);
        d2 = barrier ? 0.0 : dsc;
        if (it.last())
            it.finish();
        else
            it.step(sc, dsc, barrier);
    }
    conclude(it, d2, r, se, status);
}

// One observation of the polyserial likelihood: z standardised, (t_lo, t_hi] the thresholds around its level.
ORD_HD void polyserial_term(double z, double t_lo, double t_hi, double rho, double &score, double &dscore, bool &barrier)
{
    const double s = 1.0 - rho * rho, rs = sqrt(s), s15 = s * rs, s25 = s * s15;
    double A_lo = -INFINITY, A_hi = INFINITY, p1 = 0.0, p2 = 0.0;
    if (t_hi < INFINITY)
    {
        const double u = rho * t_hi - z, A = (t_hi - rho * z) / rs, A1 = u / s15, A2 = t_hi / s15 + 3.0 * rho * u / s25, f = phi(A);
        A_hi = A;
        p1 += f * A1;
        p2 += f * (A2 - A * A1 * A1);
    }
    if (t_lo > -INFINITY)
    {
        const double u = rho * t_lo - z, A = (t_lo - rho * z) / rs, A1 = u / s15, A2 = t_lo / s15 + 3.0 * rho * u / s25, f = phi(A);
        A_lo = A;
        p1 -= f * A1;
        p2 -= f * (A2 - A * A1 * A1);
    }
    // the difference of two tail values is formed in the tail where both are small
    const double P = A_lo > 0.0 ? Phi(-A_lo) - Phi(-A_hi) : Phi(A_hi) - Phi(A_lo);
    if (!(P >= 1e-290))  // formed in the tail, so a small value is not noise: only an underflow counts
    {
        barrier = true;
        return;
    }
    const double d1 = p1 / P;
    score += d1;
    dscore += p2 / P - d1 * d1;
}

}  // namespace ord
}  // namespace cusk
