// Per-bin algebra of one OverIVA / AuxIVA iteration with pairwise IP2 updates (which states the algorithm: the
// contract).  One launch runs the whole schedule of iteration n for every bin of every room:
//
//   n even        : (0,1), (2,3), ..., then (K-1) alone if K is odd
//   n odd, K > 2  : (0) alone, (1,2), (3,4), ..., then (K-1) alone if K is even
//   K = 2         : (0,1) in every iteration;   K = 1 : (0) alone
//
//   a single step (s)  : IP1, overiva.py:181-186
//   a pair step (a, b) : for s in {a, b}: A_s = W_hat^H V_s, P_s = A_s^-1 [e_a e_b], U_s = herm(P_s^H V_s P_s); U_b = L L^H,
//                        C = L^-1 U_a L^-H = [[p, z], [conj z, q]]; one Jacobi rotation gives C's eigenvectors q_hi, q_lo;
//                        h_a = L^-H q_hi, h_b = L^-H q_lo, each normalised in its own U; w_a = P_a h_a, w_b = P_b h_b
//   after EVERY step, when K < M: J from the orthogonality constraint, overiva.py:189-190
//
// All V_s are those of the start of the iteration (the covariance pass forms them in one pass).  Float64 throughout; W_hat is read
// from and written to the complex128 copy, its complex64 copy written alongside.  Lane layout of update_sq_kernel: one lane per
// matrix element of an MP x MP tile (identity outside M x M), 64 / (MP * MP) bins per wavefront.  M, K and the steps are run-time
// values: one kernel per MP.  No LDS, no scratch, no atomics; a bin's bits depend on its own V, Cx and W_hat alone.
#include "oiva_device.h"
#include "update_chain.h"

namespace oiva {
namespace {

using R = double;
using Z = Cx<R>;

__device__ __forceinline__ Z zconj(Z a) { return {a.re, -a.im}; }
__device__ __forceinline__ Z zscale(Z a, R s) { return {a.re * s, a.im * s}; }
__device__ __forceinline__ R zabs2(Z a) { return a.re * a.re + a.im * a.im; }
// x^H U y of 2-vectors for U = [[u00, u01], [conj u01, u11]]
__device__ __forceinline__ R quad2(Z x0, Z x1, R u00, Z u01, R u11) {
    // x^H U x = u00 |x0|^2 + u11 |x1|^2 + 2 Re(conj(x0) u01 x1)
    const Z t = cmul(zconj(x0), cmul(u01, x1));
    return u00 * zabs2(x0) + u11 * zabs2(x1) + 2. * t.re;
}

// J from the orthogonality constraint (overiva.py:96-98) into rows >= K of B = W_hat^H; C = Cx
template <int MP>
__device__ __forceinline__ void ip2_update_j(const Sq<MP, R>& sq, Z& B, const Z& C, int M, int K) {
    const int i = sq.i, j = sq.j;
    const Z Tm = sq.matmul(B, C, M);                       // rows < K: W^H Cx
    Z Gm = Tm;
    if (i >= K) Gm = Z{R(i == j ? 1 : 0), R(0)};
    Z dummy = {R(0), R(0)};
    int perm[MP];
    Z piv = {R(1), R(0)};
    sq.gauss_jordan(Gm, dummy, K, i >= K, perm, piv);
    const Z Jn = cmul(Gm, cinv(piv));                      // on row perm[m]: J[m][j-K] for j >= K
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m < K) {
            const Z row = sq.colb(Jn, perm[m]);            // lane (i, j): J[m][j-K]
            const Z tr = sq.transp(row);                   // lane (i, j): J[m][i-K]
            if (j == m && i >= K && i < M) B = zconj(tr);  // W_hat[m][i] = J[m][i-K]  ->  (W_hat^H)[i][m] = conj
        }
    }
}

// A^-1 of A = W_hat^H V (identity outside M x M)
template <int MP>
__device__ __forceinline__ Z ip2_a_inverse(const Sq<MP, R>& sq, const Z& B, const Z& V, int M) {
    Z A = sq.matmul(B, V, M);
    if (sq.i >= M || sq.j >= M) A = Z{R(sq.i == sq.j ? 1 : 0), R(0)};
    return sq.inverse_pivoted(A, M);
}

// IP1 on source s: w = A^-1 e_s, w /= sqrt(w^H V w), row s of B = w^H
template <int MP>
__device__ __forceinline__ void ip2_single(const Sq<MP, R>& sq, Z& B, const Z& V, int M, int s) {
    const int i = sq.i, j = sq.j;
    const Z Ai = ip2_a_inverse<MP>(sq, B, V, M);
    const Z wi = sq.rowb(Ai, s);                           // w_i = Ai[i][s]
    const Z wj = sq.at(Ai, j, s);                          // w_j
    const Z vw = sq.rowsum(cmul(V, wj));                   // (V w)_i  (V is the identity outside, w zero there)
    const R d = sq.allsum(j == 0 && i < M ? wi.re * vw.re + wi.im * vw.im : R(0));
    const R sc = 1. / sqrt(d);
    if (i == s && j < M) B = Z{wj.re * sc, -wj.im * sc};
}

// the two columns a, b of A_s^-1 as seen by lane (i, j) -- p?i = P[i][?], p?j = P[j][?] -- and U = herm(P^H V P)
struct Ip2Half {
    Z p0j, p1j;
    R u00, u11;
    Z u01;
};
template <int MP>
__device__ __forceinline__ Ip2Half ip2_half(const Sq<MP, R>& sq, const Z& B, const Z& V, int M, int a, int b) {
    const int i = sq.i, j = sq.j;
    const Z Ai = ip2_a_inverse<MP>(sq, B, V, M);
    Ip2Half h;
    const Z p0i = sq.rowb(Ai, a), p1i = sq.rowb(Ai, b);
    h.p0j = sq.at(Ai, j, a);
    h.p1j = sq.at(Ai, j, b);
    const Z q0 = sq.rowsum(cmul(V, h.p0j));                // (V P)[i][0]
    const Z q1 = sq.rowsum(cmul(V, h.p1j));                // (V P)[i][1]
    const bool on = j == 0 && i < M;                       // one lane per row adds its term
    const Z c0 = zconj(p0i), c1 = zconj(p1i);
    const Z t00 = cmul(c0, q0), t01 = cmul(c0, q1), t10 = cmul(c1, q0), t11 = cmul(c1, q1);
    const R z = R(0);
    const R s00 = sq.allsum(on ? t00.re : z);
    const R s11 = sq.allsum(on ? t11.re : z);
    const R s01r = sq.allsum(on ? t01.re : z), s01i = sq.allsum(on ? t01.im : z);
    const R s10r = sq.allsum(on ? t10.re : z), s10i = sq.allsum(on ? t10.im : z);
    h.u00 = s00;                                           // the Hermitian part: real diagonal, (U01 + conj U10) / 2
    h.u11 = s11;
    h.u01 = Z{0.5 * (s01r + s10r), 0.5 * (s01i - s10i)};
    return h;
}

// the pair step (a, b), a < b
template <int MP>
__device__ __forceinline__ void ip2_pair(const Sq<MP, R>& sq, Z& B, const Z& Va, const Z& Vb, int M, int a, int b) {
    const int i = sq.i, j = sq.j;
    const Ip2Half ha = ip2_half<MP>(sq, B, Va, M, a, b);
    const Ip2Half hb = ip2_half<MP>(sq, B, Vb, M, a, b);
    // U_b = L L^H;  Li = L^-1 = [[m00, 0], [m10, m11]]
    const R l00 = sqrt(hb.u00);
    const Z l10 = zscale(zconj(hb.u01), 1. / l00);
    const R l11 = sqrt(hb.u11 - zabs2(l10));
    const R m00 = 1. / l00, m11 = 1. / l11;
    const Z m10 = zscale(l10, -(m00 * m11));
    // C = Li U_a Li^H = [[p, z], [conj z, q]]
    const Z ua10 = zconj(ha.u01);
    const Z t00 = {m00 * ha.u00, R(0)};
    const Z t01 = zscale(ha.u01, m00);
    Z t10 = zscale(m10, ha.u00);
    t10.re += m11 * ua10.re;
    t10.im += m11 * ua10.im;
    Z t11 = cmul(m10, ha.u01);
    t11.re += m11 * ha.u11;
    const Z cm10 = zconj(m10);
    const R p = t00.re * m00;
    Z z = cmul(t00, cm10);
    z.re += t01.re * m11;
    z.im += t01.im * m11;
    const R q = cmul(t10, cm10).re + t11.re * m11;
    // one rotation: the eigenpairs of C
    const R az = sqrt(zabs2(z));
    R c = 1., s = 0., t = 0.;
    Z phi = {R(1), R(0)};
    if (!(az == 0.)) {
        phi = zscale(z, 1. / az);
        const R tau = (q - p) / (2. * az);
        t = tau == 0. ? 1. : (tau > 0. ? 1. : -1.) / (fabs(tau) + sqrt(1. + tau * tau));
        c = 1. / sqrt(1. + t * t);
        s = t * c;
    }
    const R lam1 = p - t * az, lam2 = q + t * az;
    const Z v10 = {c, R(0)}, v11 = zscale(zconj(phi), -s);   // v1 = (c, -s conj(phi))
    const Z v20 = zscale(phi, s), v21 = {c, R(0)};           // v2 = (s phi, c)
    const bool first = lam1 >= lam2;                         // q_hi: the larger eigenvalue, a tie takes v1
    const Z hi0 = {first ? v10.re : v20.re, first ? v10.im : v20.im}, hi1 = {first ? v11.re : v21.re, first ? v11.im : v21.im};
    const Z lo0 = {first ? v20.re : v10.re, first ? v20.im : v10.im}, lo1 = {first ? v21.re : v11.re, first ? v21.im : v11.im};
    // h = L^-H q = Li^H q = (m00 q0 + conj(m10) q1, m11 q1), normalised in its own U
    Z ha0 = zscale(hi0, m00), hb0 = zscale(lo0, m00);
    cfma(ha0, cm10, hi1);
    cfma(hb0, cm10, lo1);
    Z ha1 = zscale(hi1, m11), hb1 = zscale(lo1, m11);
    const R na = 1. / sqrt(quad2(ha0, ha1, ha.u00, ha.u01, ha.u11));
    const R nb = 1. / sqrt(quad2(hb0, hb1, hb.u00, hb.u01, hb.u11));
    ha0 = zscale(ha0, na), ha1 = zscale(ha1, na);
    hb0 = zscale(hb0, nb), hb1 = zscale(hb1, nb);
    // w_a = P_a h_a, w_b = P_b h_b: entry j on every lane of column j; rows a and b of B = their conjugates
    Z wa = cmul(ha.p0j, ha0), wb = cmul(hb.p0j, hb0);
    cfma(wa, ha.p1j, ha1);
    cfma(wb, hb.p1j, hb1);
    if (j < M) {
        if (i == a) B = zconj(wa);
        if (i == b) B = zconj(wb);
    }
}

template <int MP>
__global__ __launch_bounds__(kBlock) void ip2_update_kernel(UpdateArgs a, int parity) {
    constexpr int G = MP * MP;
    const int tid = threadIdx.x;
    const Sq<MP, R> sq(tid % G);
    const int i = sq.i, j = sq.j;
    const int f_raw = blockIdx.x * (kBlock / G) + tid / G;
    const bool fvalid = f_raw < a.F;
    const int f = fvalid ? f_raw : a.F - 1;        // (a bin past the end repeats the last one and stores nothing)
    const int M = a.M, K = a.K;
    const int NA = M * M;
    const bool in = i < M && j < M;
    const Z zero = {R(0), R(0)};
    const Z eye = {R(i == j ? 1 : 0), R(0)};

    Z B = eye;                                     // B[i][j] = (W_hat^H)[i][j] = conj(W_hat[j][i]); identity outside M x M
    if (in) {
        const double2 v = a.What64[((size_t)f * M + j) * M + i];
        B = {v.x, -v.y};
    }
    int off = 0;
    float sgn = 0.f;
    if (in) herm_offsets(M, i, j, off, sgn);
    Z C = zero;                                    // Cx
    if (in && K < M) {
        const double* p = a.Cx + (size_t)f * NA + off;
        C.re = p[0];
        if (sgn != 0.f) C.im = R(sgn) * p[1];
    }
    const R invT = R(1) / R(update_frames(a, f));  // T and split count of the bin's own room
    const int nsplit = update_nsplit(a, f);
    const double* vpart = static_cast<const double*>(a.Vpart);
    auto load_v = [&](int s) {
        Z V = eye;
        if (in) {
            double sr, si;
            sum_vpart_t(vpart, ((size_t)f * K + s) * NA + off, (size_t)a.F * K * NA, nsplit, sr, si);
            V = {sr * invT, sgn != 0.f ? si * R(sgn) * invT : R(0)};
        }
        return V;
    };

    int s = 0;
    if (K == 1 || (K > 2 && parity)) {
        ip2_single<MP>(sq, B, load_v(0), M, 0);
        if (K < M) ip2_update_j<MP>(sq, B, C, M, K);
        s = 1;
    }
    for (; s + 1 < K; s += 2) {
        const Z Va = load_v(s), Vb = load_v(s + 1);
        ip2_pair<MP>(sq, B, Va, Vb, M, s, s + 1);
        if (K < M) ip2_update_j<MP>(sq, B, C, M, K);
    }
    if (s < K) {
        ip2_single<MP>(sq, B, load_v(s), M, s);
        if (K < M) ip2_update_j<MP>(sq, B, C, M, K);
    }

    if (fvalid && in) {
        const size_t o = ((size_t)f * M + j) * M + i;
        a.What64[o] = make_double2(B.re, -B.im);
        a.What[o] = make_float2((float)B.re, (float)-B.im);
    }
}

}  // namespace

// a: What, What64, Cx, Vpart (float64), T / nsplit or the problem table, F = all bins of the batch, M, K, wscale_bins = bins of a
// room; the activation has applied the scale of W in float64 (a.wscale is not read)
hipError_t launch_ip2_update(hipStream_t s, const UpdateArgs& a, int iteration) {
    if (a.M < 1 || a.M > 8 || a.K < 1 || a.K > a.M || a.F < 1 || !a.What64 || !a.vpart_f64 || iteration < 0) return hipErrorInvalidValue;
    const int mp = a.M <= 2 ? 2 : (a.M <= 4 ? 4 : 8);
    const dim3 grid((unsigned)ceil_div(a.F, kBlock / (mp * mp))), block(kBlock);
    const int parity = iteration & 1;
    switch (mp) {
        case 2: hipLaunchKernelGGL(ip2_update_kernel<2>, grid, block, 0, s, a, parity); break;
        case 4: hipLaunchKernelGGL(ip2_update_kernel<4>, grid, block, 0, s, a, parity); break;
        default: hipLaunchKernelGGL(ip2_update_kernel<8>, grid, block, 0, s, a, parity); break;
    }
    return hipGetLastError();
}

}  // namespace oiva
