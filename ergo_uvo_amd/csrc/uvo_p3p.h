// uvo_p3p.h -- the three-point pose solver of the PnP-RANSAC kernels (device side), after Gao, Hou, Tang and Cheng, "Complete solution
// classification for the perspective-three-point problem" (PAMI 2003), as reached by cv::solvePnPRansac(flags = SOLVEPNP_P3P) at
// visual_odometry.h:647-648 and by every solvePnPRansac call on exactly four points.  Written from the paper: the operation order is this
// file's own, not OpenCV's p3p.cpp.
//
//   A, B, C      the object points, a = |BC|, b = |AC|, c = |AB|;  fA, fB, fC the unit bearings of their images
//   p, q, r      2 cos of the angles (fB, fC), (fA, fC), (fA, fB);  X, Y, Z the unknown distances camera -> A, B, C
//   law of cosines:   Y^2 + Z^2 - p Y Z = a^2,   X^2 + Z^2 - q X Z = b^2,   X^2 + Y^2 - r X Y = c^2
//   with x = X / Z, y = Y / Z, v = c^2 / Z^2 = x^2 + y^2 - r x y, a' = a^2 / c^2, b' = b^2 / c^2:
//       E1: (1 - a') y^2 - a' x^2 - p y + a' r x y + 1 = 0
//       E2: (1 - b') x^2 - b' y^2 - q x + b' r x y + 1 = 0
//   b' E1 + (1 - a') E2 is linear in y:   b' (r x - p) y + N(x) = 0,   N = (1 - a' - b') x^2 - (1 - a') q x + (1 - a' + b')
//   and y = N / (b' L), L = p - r x, put into b' L^2 E2 leaves the quartic   -N^2 + b' r x N L + b' M L^2 = 0,   M = (1 - b') x^2 - q x + 1.
//   Every real root x > 0 with y > 0 and v > 0 gives Z = c / sqrt(v), X = x Z, Y = y Z, the camera-frame points X fA, Y fB, Z fC, and
//   the pose is their absolute orientation against A, B, C (Horn 1987: the unit quaternion is the eigenvector of the largest
//   eigenvalue of a symmetric 4 x 4 matrix, found by cyclic Jacobi).
// Everything is fp64 in registers: every array index below is a compile-time constant after unrolling.
#pragma once
#include <math.h>
#include <float.h>

namespace uvo {

// Real roots of x^4 + a3 x^3 + a2 x^2 + a1 x + a0 by Ferrari's method: the depressed quartic u^4 + P u^2 + Q u + R (x = u - a3 / 4) is
// the difference of two squares (u^2 + P/2 + m)^2 - (s u - Q / (2 s))^2, s = sqrt(2 m), for a positive root m of the resolvent cubic
// m^3 + P m^2 + (P^2/4 - R) m - Q^2/8.  Slots 0, 1 hold the roots of the first quadratic factor, 2, 3 those of the second; the return
// value is the mask of the slots filled.  A discriminant that is negative by rounding only (a double root) counts as zero.
__host__ __device__ inline int p3p_quartic_roots(double a3, double a2, double a1, double a0, double* x)
{
    const double h = 0.25 * a3;
    const double P = a2 - 6. * h * h;
    const double Q = a1 - 2. * a2 * h + 8. * h * h * h;
    const double R = a0 - a1 * h + a2 * h * h - 3. * h * h * h * h;
    const double scale = fabs(P) + sqrt(fabs(R)) + cbrt(Q * Q);          // ~ u^2 of the roots
    double s, c1, c2;                                                     // the factors u^2 - s u + c1 and u^2 + s u + c2
    if (fabs(Q) <= 1e-14 * scale * sqrt(scale)) {                         // biquadratic: u^2 = (-P +- sqrt(P^2 - 4 R)) / 2
        double d = P * P - 4. * R;
        if (d < 0) { if (d < -1e-12 * (P * P + fabs(R))) return 0; d = 0; }
        const double sd = sqrt(d);
        // (u^2 - w1)(u^2 - w2): as "factors" u^2 - 0 u - w1 and u^2 + 0 u - w2
        s = 0; c1 = -0.5 * (-P + sd); c2 = -0.5 * (-P - sd);
    } else {
        // the largest real root of the resolvent: positive, because the cubic is -Q^2 / 8 < 0 at m = 0
        const double cb = P, cc = 0.25 * P * P - R, cd = -0.125 * Q * Q;
        const double pp = cc - cb * cb / 3., qq = 2. * cb * cb * cb / 27. - cb * cc / 3. + cd;
        const double disc = 0.25 * qq * qq + pp * pp * pp / 27.;
        double w;
        if (disc > 0) { const double sd = sqrt(disc); w = cbrt(-0.5 * qq + sd) + cbrt(-0.5 * qq - sd); }
        else {
            const double k = sqrt(-pp / 3.);
            double arg = k > 0 ? -0.5 * qq / (k * k * k) : 1.;
            arg = arg > 1. ? 1. : arg < -1. ? -1. : arg;
            w = 2. * k * cos(acos(arg) / 3.);
        }
        double m = w - cb / 3.;
        for (int it = 0; it < 3; it++) {                                  // Newton on the cubic itself: the closed form loses digits to cancellation
            const double f = ((m + cb) * m + cc) * m + cd, df = (3. * m + 2. * cb) * m + cc;
            if (!(fabs(df) > 0)) break;
            const double mn = m - f / df;
            if (!(mn > 0)) break;
            m = mn;
        }
        if (!(m > 0)) return 0;
        s = sqrt(2. * m);
        const double e = Q / (2. * s);
        c1 = 0.5 * P + m + e; c2 = 0.5 * P + m - e;
    }
    int mask = 0;
    {
        double d = s * s - 4. * c1;
        if (d < 0 && d >= -1e-12 * (s * s + fabs(c1))) d = 0;
        if (d >= 0) { const double sd = sqrt(d); x[0] = 0.5 * (s + sd) - h; x[1] = 0.5 * (s - sd) - h; mask |= 3; }
    }
    {
        double d = s * s - 4. * c2;
        if (d < 0 && d >= -1e-12 * (s * s + fabs(c2))) d = 0;
        if (d >= 0) { const double sd = sqrt(d); x[2] = 0.5 * (-s + sd) - h; x[3] = 0.5 * (-s - sd) - h; mask |= 12; }
    }
    // two Newton steps on the quartic as given (a step is kept only where the derivative is not small: never at a double root)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (!(mask >> k & 1)) continue;
        double r = x[k];
        for (int it = 0; it < 2; it++) {
            const double f = (((r + a3) * r + a2) * r + a1) * r + a0;
            const double df = ((4. * r + 3. * a3) * r + 2. * a2) * r + a1;
            const double mag = ((fabs(4. * r) + fabs(3. * a3)) * fabs(r) + fabs(2. * a2)) * fabs(r) + fabs(a1);
            if (!(fabs(df) > 1e-6 * mag)) break;
            r -= f / df;
        }
        x[k] = r;
    }
    return mask;
}

// Absolute orientation of three point pairs (Horn 1987): R, t with cam_i = R obj_i + t in the least-squares sense, R a rotation.
__host__ __device__ inline void p3p_align(const double (*obj)[3], const double (*cam)[3], double* R, double* t, double* quat)
{
    double oc[3], cc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { oc[k] = (obj[0][k] + obj[1][k] + obj[2][k]) / 3.; cc[k] = (cam[0][k] + cam[1][k] + cam[2][k]) / 3.; }
    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            double s = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) s += (obj[i][a] - oc[a]) * (cam[i][b] - cc[b]);
            S[a][b] = s;
        }
    double A[4][4], V[4][4];
    A[0][0] = S[0][0] + S[1][1] + S[2][2]; A[1][1] = S[0][0] - S[1][1] - S[2][2]; A[2][2] = -S[0][0] + S[1][1] - S[2][2]; A[3][3] = -S[0][0] - S[1][1] + S[2][2];
    A[0][1] = A[1][0] = S[1][2] - S[2][1]; A[0][2] = A[2][0] = S[2][0] - S[0][2]; A[0][3] = A[3][0] = S[0][1] - S[1][0];
    A[1][2] = A[2][1] = S[0][1] + S[1][0]; A[1][3] = A[3][1] = S[2][0] + S[0][2]; A[2][3] = A[3][2] = S[1][2] + S[2][1];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1. : 0.;
    for (int sweep = 0; sweep < 16; sweep++) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[0][3] * A[0][3] + A[1][2] * A[1][2] + A[1][3] * A[1][3] + A[2][3] * A[2][3];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2] + A[3][3] * A[3][3];
        if (!(off > 1e-34 * dia)) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                if (apq == 0) continue;
                const double th = (A[q][q] - A[p][p]) / (2. * apq);
                const double tt = (th >= 0 ? 1. : -1.) / (fabs(th) + sqrt(th * th + 1.));
                const double c = 1. / sqrt(tt * tt + 1.), s = tt * c;
#pragma unroll
                for (int k = 0; k < 4; k++) { const double u = A[k][p], w = A[k][q]; A[k][p] = c * u - s * w; A[k][q] = s * u + c * w; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double u = A[p][k], w = A[q][k]; A[p][k] = c * u - s * w; A[q][k] = s * u + c * w; }
#pragma unroll
                for (int k = 0; k < 4; k++) { const double u = V[k][p], w = V[k][q]; V[k][p] = c * u - s * w; V[k][q] = s * u + c * w; }
            }
    }
    double best = A[0][0], qw = V[0][0], qx = V[1][0], qy = V[2][0], qz = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; j++) if (A[j][j] > best) { best = A[j][j]; qw = V[0][j]; qx = V[1][j]; qy = V[2][j]; qz = V[3][j]; }
    const double in = 1. / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= in; qx *= in; qy *= in; qz *= in;
    if (qw < 0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    R[0] = 1. - 2. * (qy * qy + qz * qz); R[1] = 2. * (qx * qy - qw * qz); R[2] = 2. * (qx * qz + qw * qy);
    R[3] = 2. * (qx * qy + qw * qz); R[4] = 1. - 2. * (qx * qx + qz * qz); R[5] = 2. * (qy * qz - qw * qx);
    R[6] = 2. * (qx * qz - qw * qy); R[7] = 2. * (qy * qz + qw * qx); R[8] = 1. - 2. * (qx * qx + qy * qy);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = cc[k] - (R[3*k] * oc[0] + R[3*k + 1] * oc[1] + R[3*k + 2] * oc[2]);
    quat[0] = qw; quat[1] = qx; quat[2] = qy; quat[3] = qz;
}

// the rotation vector of a unit quaternion with w >= 0: angle 2 atan2(|v|, w) about v
__host__ __device__ inline void p3p_quat2rvec(const double* q, double* rv)
{
    const double sn = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double k = sn > 0 ? 2. * atan2(sn, q[0]) / sn : 0.;
    rv[0] = k * q[1]; rv[1] = k * q[2]; rv[2] = k * q[3];
}

// P3P on points 0..2 of a four-point subset, the fourth point choosing among the solutions (smallest squared reprojection error in
// normalised image coordinates; the first in root order on a tie).  obj: object points; img: normalised image points (x, y) of a
// camera looking along +z.  false: no admissible solution -- object points (nearly) collinear, bearings (nearly) coplanar, no real
// positive root with positive distances.
__host__ __device__ inline bool p3p_solve4(const double (*obj)[3], const double (*img)[2], double* rvec, double* tvec)
{
    double f[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double in = 1. / sqrt(img[i][0] * img[i][0] + img[i][1] * img[i][1] + 1.);
        f[i][0] = img[i][0] * in; f[i][1] = img[i][1] * in; f[i][2] = in;
    }
    double ab[3], ac[3], bc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { ab[k] = obj[1][k] - obj[0][k]; ac[k] = obj[2][k] - obj[0][k]; bc[k] = obj[2][k] - obj[1][k]; }
    const double c2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], b2 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2],
                 a2 = bc[0] * bc[0] + bc[1] * bc[1] + bc[2] * bc[2];
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    if (!(nx * nx + ny * ny + nz * nz > 1e-20 * c2 * b2)) return false;          // collinear (or coincident) object points: no unique pose
    const double trip = f[0][0] * (f[1][1] * f[2][2] - f[1][2] * f[2][1]) - f[0][1] * (f[1][0] * f[2][2] - f[1][2] * f[2][0])
                      + f[0][2] * (f[1][0] * f[2][1] - f[1][1] * f[2][0]);
    if (!(fabs(trip) > 1e-12)) return false;                                     // coplanar bearings (the three images on one line)
    const double p = 2. * (f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2]);
    const double q = 2. * (f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2]);
    const double r = 2. * (f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2]);
    const double a = a2 / c2, b = b2 / c2, c = sqrt(c2);
    // N, L, M as polynomials in x (index = power)
    const double N0 = 1. - a + b, N1 = -(1. - a) * q, N2 = 1. - a - b;
    const double L0 = p, L1 = -r;
    const double M0 = 1., M1 = -q, M2 = 1. - b;
    // -N^2
    double k0 = -N0 * N0, k1 = -2. * N0 * N1, k2 = -(2. * N0 * N2 + N1 * N1), k3 = -2. * N1 * N2, k4 = -N2 * N2;
    // + b r x N L
    const double NL0 = N0 * L0, NL1 = N0 * L1 + N1 * L0, NL2 = N1 * L1 + N2 * L0, NL3 = N2 * L1;
    const double br = b * r;
    k1 += br * NL0; k2 += br * NL1; k3 += br * NL2; k4 += br * NL3;
    // + b M L^2
    const double LL0 = L0 * L0, LL1 = 2. * L0 * L1, LL2 = L1 * L1;
    k0 += b * (M0 * LL0); k1 += b * (M0 * LL1 + M1 * LL0); k2 += b * (M0 * LL2 + M1 * LL1 + M2 * LL0); k3 += b * (M1 * LL2 + M2 * LL1); k4 += b * (M2 * LL2);
    if (!(fabs(k4) > 1e-14 * (fabs(k0) + fabs(k1) + fabs(k2) + fabs(k3)))) return false;     // a root at infinity: the paper's degenerate branch, not served
    double xs[4];
    const double ik4 = 1. / k4;
    const int mask = p3p_quartic_roots(k3 * ik4, k2 * ik4, k1 * ik4, k0 * ik4, xs);
    bool found = false;
    double best_err = 0;
    for (int k = 0; k < 4; k++) {
        double x = k == 0 ? xs[0] : k == 1 ? xs[1] : k == 2 ? xs[2] : xs[3];
        if (!(mask >> k & 1) || !(x > 0)) continue;
        const double L = L0 + L1 * x, Nx = N0 + (N1 + N2 * x) * x;
        double y;
        if (fabs(L) > 1e-9 * (fabs(L0) + fabs(L1 * x))) y = Nx / (b * L);
        else {
            // x = p / r: the linear relation is void there and y is a root of E1 itself; the one that also satisfies E2
            const double qa = 1. - a, qb = a * r * x - p, qc = 1. - a * x * x;
            if (!(fabs(qa) > 0)) continue;
            double d = qb * qb - 4. * qa * qc;
            if (d < 0) continue;
            d = sqrt(d);
            const double y1 = (-qb + d) / (2. * qa), y2 = (-qb - d) / (2. * qa);
            const double Mx = M0 + (M1 + M2 * x) * x;
            const double e1 = fabs(-b * y1 * y1 + br * x * y1 + Mx), e2 = fabs(-b * y2 * y2 + br * x * y2 + Mx);
            y = e1 <= e2 ? y1 : y2;
            if (!((e1 <= e2 ? e1 : e2) <= 1e-9 * (fabs(Mx) + b * y * y + 1.))) continue;
        }
        if (!(y > 0)) continue;
        const double v = x * x + y * y - r * x * y;
        if (!(v > 0)) continue;
        double Z = c / sqrt(v), X = x * Z, Y = y * Z;
        // The quartic's coefficients carry the cancellation of their long products; two Newton steps on the three law-of-cosines
        // equations themselves bring a simple solution back to rounding error (a step is skipped where the Jacobian is singular).
        for (int it = 0; it < 2; it++) {
            const double F1 = Y * Y + Z * Z - p * Y * Z - a2, F2 = X * X + Z * Z - q * X * Z - b2, F3 = X * X + Y * Y - r * X * Y - c2;
            const double j12 = 2. * Y - p * Z, j13 = 2. * Z - p * Y, j21 = 2. * X - q * Z, j23 = 2. * Z - q * X, j31 = 2. * X - r * Y, j32 = 2. * Y - r * X;
            const double det = j12 * j23 * j31 + j13 * j21 * j32;
            if (!(fabs(det) > 1e-9 * c2 * c)) break;
            const double id = 1. / det;
            // -J^{-1} F by cofactors, J = [0 j12 j13; j21 0 j23; j31 j32 0]
            const double dX = (j23 * j32 * F1 - j13 * j32 * F2 - j12 * j23 * F3) * id;
            const double dY = (-j23 * j31 * F1 + j13 * j31 * F2 - j13 * j21 * F3) * id;
            const double dZ = (-j21 * j32 * F1 - j12 * j31 * F2 + j12 * j21 * F3) * id;
            X += dX; Y += dY; Z += dZ;
        }
        if (!(X > 0 && Y > 0 && Z > 0)) continue;
        double cam[3][3];
#pragma unroll
        for (int j = 0; j < 3; j++) { cam[0][j] = X * f[0][j]; cam[1][j] = Y * f[1][j]; cam[2][j] = Z * f[2][j]; }
        double R[9], t[3], quat[4];
        p3p_align(obj, cam, R, t, quat);
        const double px = R[0] * obj[3][0] + R[1] * obj[3][1] + R[2] * obj[3][2] + t[0];
        const double py = R[3] * obj[3][0] + R[4] * obj[3][1] + R[5] * obj[3][2] + t[1];
        const double pz = R[6] * obj[3][0] + R[7] * obj[3][1] + R[8] * obj[3][2] + t[2];
        const double ex = px / pz - img[3][0], ey = py / pz - img[3][1];
        const double err = ex * ex + ey * ey;
        if (!(err == err)) continue;
        if (!found || err < best_err) {
            found = true; best_err = err;
            p3p_quat2rvec(quat, rvec);
            tvec[0] = t[0]; tvec[1] = t[1]; tvec[2] = t[2];
        }
    }
    return found;
}

}  // namespace uvo
