// Student's t for the per-row kernels (textually included by fokl_hip.hip ahead of fokl_score_device.inc and
// fokl_predictive_device.inc): the constants the host forms, Gamma(a + 1/2) / Gamma(a), and student_terms, CDF and density
// at one point.  The statement is fokl_gpy_amd/predictive.py: student_terms and _Student, operation for operation.
//
// T_nu(t) through the regularised incomplete beta function: with r = t^2 / nu, x = 1 / (1 + r) = nu / (nu + t^2) and
// y = r x = t^2 / (nu + t^2), P(|T| > |t|) = I_x(a, 1/2), a = nu / 2, and I_x(a, 1/2) = 1 - I_y(1/2, a).  Both have the
// continued fraction I_z(p, q) = z^p (1 - z)^q / (p B(p, q)) h, h = 1 / (1 + d_1 / (1 + d_2 / (1 + ...))), d_n = coefficient_n z.
// Since x^a y^(1/2) / B(a, 1/2) = f_nu(t) |t|, ONE exp gives the density and both prefactors:
//   direct   (x <  (a + 1) / (a + 5/2)):  T = v for t < 0, 1 - v otherwise, v = (0.5 / a) f |t| h     (the lower tail itself)
//   mirrored (elsewhere):                  T = 0.5 + f t h
// h is evaluated by the fraction's forward recurrence A_n = A_{n-1} + d_{n-1} A_{n-2} (B likewise), two steps per iteration,
// no division until h = A / B at the end: every |d_n| is below 1, so A and B stay within 2^(2 ST_ITERS) and need no
// rescaling.  The coefficients without their argument come from the host as a table [4][ST_ITERS + 1] (direct even, direct
// odd, mirrored even, mirrored odd), read with a wave-uniform index.  A lane whose fraction has converged (|A_n B_{n-1} -
// A_{n-1} B_n| <= ST_EPS |A_n B_{n-1}|) keeps its values and waits; the loop ends when no lane of the wavefront is live or at
// ST_ITERS, the fixed bound that the statement has too: within it every argument converges for every nu in [1,
// FOKL_PREDICTIVE_NU_MAX].  All lanes of the wavefront must call student_terms together (__any).

namespace fokl {

constexpr int ST_ITERS = FOKL_PREDICTIVE_STUDENT_ITERATIONS;
constexpr int ST_ROW = ST_ITERS + 1;             // entries of one of the table's four rows
constexpr double ST_EPS = 0x1p-51;

struct StudentArgs {
    double inu, hp, cn, xb, ha;                  // 1 / nu, a + 1/2, the density at 0, the branch point, 0.5 / a
};

// Gamma(a + 1/2) / Gamma(a) for a >= 1/2, as ONE number: tgamma twice below 80, above it sqrt(a) times exp of the asymptotic
// series.  The difference of two lgamma loses every digit that their size has in front of the point (score.gamma_ratio).
static double student_gamma_ratio(double a)
{
    if (a < 80.0) return std::tgamma(a + 0.5) / std::tgamma(a);
    const double r = 1.0 / (a * a);
    return std::sqrt(a) * std::exp((-1.0 / 8.0 + (1.0 / 192.0 + (-1.0 / 640.0 + 17.0 / 14336.0 * r) * r) * r) / a);
}

// the constants and the table [4][ST_ROW] of predictive._Student
static StudentArgs student_fill(double nu, double *tab)
{
    const double a = 0.5 * nu;
    StudentArgs k;
    k.inu = 1.0 / nu;
    k.hp = a + 0.5;
    k.cn = student_gamma_ratio(a) / std::sqrt(nu * M_PI);
    k.xb = (a + 1.0) / (a + 2.5);
    k.ha = 0.5 / a;
    for (int i = 0; i < ST_ROW; ++i) {
        const double m = (double)i, m2 = 2.0 * m;
        tab[i] = i ? m * (0.5 - m) / ((a + m2 - 1.0) * (a + m2)) : 0.0;
        tab[ST_ROW + i] = -(a + m) * (a + 0.5 + m) / ((a + m2) * (a + m2 + 1.0));
        tab[2 * ST_ROW + i] = m * (a - m) / ((m2 - 0.5) * (m2 + 0.5));
        tab[3 * ST_ROW + i] = -(0.5 + m) * (a + 0.5 + m) / ((m2 + 0.5) * (m2 + 1.5));
    }
    return k;
}

// T = T_nu(t), f = f_nu(t)
__device__ __forceinline__ void student_terms(double t, const StudentArgs &k, const double *__restrict__ tab, double &T, double &f)
{
    const double r = (t * t) * k.inu;
    const double L = log1p(r);
    const double x = 1.0 / (1.0 + r);
    f = k.cn * exp(-k.hp * L);
    const bool direct = x < k.xb;
    const double z = direct ? x : r * x;
    double A0 = 1.0, B0 = 1.0, A1 = 1.0, B1 = 1.0 + (direct ? tab[ST_ROW] : tab[3 * ST_ROW]) * z;
    bool live = true;
#pragma unroll 1
    for (int m = 1; m <= ST_ITERS; ++m) {
        if (!__any(live)) break;                     // wave uniform; otherwise the bound alone ends the loop
        const double dE = (direct ? tab[m] : tab[2 * ST_ROW + m]) * z;
        const double dO = (direct ? tab[ST_ROW + m] : tab[3 * ST_ROW + m]) * z;
        const double A2 = A1 + dE * A0, B2 = B1 + dE * B0;
        const double A3 = A2 + dO * A1, B3 = B2 + dO * B1;
        if (live) {
            A0 = A2;
            B0 = B2;
            A1 = A3;
            B1 = B3;
        }
        live = live && !(fabs(A3 * B2 - A2 * B3) <= ST_EPS * fabs(A3 * B2));
    }
    const double g = f * t * (A1 / B1);
    const double v = k.ha * fabs(g);
    T = direct ? (t < 0.0 ? v : 1.0 - v) : 0.5 + g;
}

}  // namespace fokl
