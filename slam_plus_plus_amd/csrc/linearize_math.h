// linearize_math.h -- the edge models and manifold updates of linearize.hip as plain functions of one edge or one vertex:
// no memory layout, no thread index.  They compile for the device and for the host alike, so that a CPU program can run
// the very arithmetic the kernels run (tests/linearize_math_driver.cpp).
//
// The definitions (the reference's members they stand for are named in include/slampp_hip.h):
//   SE(2) pose-pose   h = (R^T(th0) (p1 - p0), fmod(th1 - th0, 2 pi)), err = z - h with the angle folded to the nearest turn,
//                     Jacobians with respect to an additive perturbation of the state;
//   SE(3) pose-pose   h = (R0^T (t1 - t0), Log(R0^T R1)), err = (z_t - h_t, Log(Exp(z_r) Exp(h_r)^T)), Log the principal
//                     logarithm; J0 = dh(x0 (+) e, x1) / de, J1 = dh(x0, x1 (+) e) / de at e = 0 with
//                     x (+) e: t <- t + R e_t, R <- R Exp(e_r):
//                       J0 = [-I, [h_t]x; 0, -Jl^-1(h_r)],  J1 = [R0^T R1, 0; 0, Jr^-1(h_r)],
//                       Jl^-1(phi) = I - 1/2 [phi]x + c(theta) [phi]x^2,  Jr^-1(phi) = Jl^-1(-phi),
//                       c(theta) = 1 / theta^2 - cot(theta / 2) / (2 theta)      ( = 1/theta^2 - (1 + cos) / (2 theta sin) )
//   camera-point      x = R X + t, p = (fx x / z, fy y / z), projection = c + (1 + k' |p|^2) p with k' = k / ((fx + fy) / 2),
//                     err = z - projection; the camera moves by the SE(3) (+) above (dx/de = R [I, -[X]x]), the point
//                     additively (dx/dX = R).
//   pose-landmark 2D  h = (max(|l - p|, 1e-5), fmod(atan2(l - p) - th, 2 pi)), err = z - h with the angle folded; additive Jacobians
//   pose-landmark 3D  h = R0^T (X - t0), err = z - h; J0 = [-I, [h]x] under the SE(3) (+), J1 = R0^T
//   stereo camera     the camera-point projection with a radial term linear in |p|, and u of the same projection of
//                     x - (baseline, 0, 0): DESIGN.md section 4.12
// Rotations travel as unit quaternions (w >= 0 picks the principal logarithm, and a small angle keeps its relative accuracy,
// which a rotation matrix's off-diagonal differences would not).
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SLAMPP_LIN_FN __host__ __device__ __forceinline__
#else
#define SLAMPP_LIN_FN inline
#endif

namespace slampp {
namespace lin {

// below this angle c(theta) comes from its series 1/12 + theta^2/720 + theta^4/30240 + theta^6/1209600 (the first term left
// out, theta^8 / 47900160, is 8e-19 there); above it the closed form loses at most 1e-16 / theta^2 of 1/12, which the factor
// [phi]x^2 = O(theta^2) behind it takes back
#define SLAMPP_LIN_SERIES_BELOW 0.05

SLAMPP_LIN_FN double two_pi() { return 2 * 3.14159265358979323846; }

// the angle modulo 2 pi, in (-2 pi, 2 pi), with the sign of the angle; 0 for an infinity or a NaN
SLAMPP_LIN_FN double clamp_angle_2pi(double f_angle)
{
	return (f_angle - f_angle == 0)? fmod(f_angle, two_pi()) : 0;
}

// of e, e - 2 pi, e + 2 pi (e the error modulo 2 pi) the one of the least magnitude
SLAMPP_LIN_FN double clamp_angular_error_2pi(double f_error)
{
	const double a = clamp_angle_2pi(f_error), b = a - two_pi(), c = a + two_pi();
	const double m = (fabs(a) < fabs(b))? a : b;
	return (fabs(m) < fabs(c))? m : c;
}

struct TQuat {
	double w, x, y, z;
};

// the unit quaternion of Exp(phi), any |phi|
SLAMPP_LIN_FN TQuat quat_exp(const double *phi)
{
	const double f_theta = sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
	const double f_half = .5 * f_theta, s = (f_theta > 0)? sin(f_half) / f_theta : .5;
	TQuat q = {cos(f_half), s * phi[0], s * phi[1], s * phi[2]};
	return q;
}

SLAMPP_LIN_FN TQuat quat_mul(const TQuat &a, const TQuat &b)
{
	TQuat q = {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
		a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
	return q;
}

SLAMPP_LIN_FN TQuat quat_conj(const TQuat &a)
{
	TQuat q = {a.w, -a.x, -a.y, -a.z};
	return q;
}

// the principal logarithm (angle in [0, pi]) of the rotation of q or of -q, which are the same rotation
SLAMPP_LIN_FN void quat_log(const TQuat &q, double *phi)
{
	const double f_sign = (q.w < 0)? -1.0 : 1.0, w = f_sign * q.w;
	const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
	const double k = f_sign * ((n > 0)? 2 * atan2(n, w) / n : 2 / w);
	phi[0] = k * q.x; phi[1] = k * q.y; phi[2] = k * q.z;
}

// R (column-major 3 x 3) of a unit quaternion
SLAMPP_LIN_FN void quat_to_rot(const TQuat &q, double *R)
{
	const double xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xy = q.x * q.y, xz = q.x * q.z, yz = q.y * q.z,
		wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
	R[0] = 1 - 2 * (yy + zz); R[3] = 2 * (xy - wz);     R[6] = 2 * (xz + wy);
	R[1] = 2 * (xy + wz);     R[4] = 1 - 2 * (xx + zz); R[7] = 2 * (yz - wx);
	R[2] = 2 * (xz - wy);     R[5] = 2 * (yz + wx);     R[8] = 1 - 2 * (xx + yy);
}

SLAMPP_LIN_FN double inv_jacobian_c(double f_theta)
{
	const double t2 = f_theta * f_theta;
	if(f_theta < SLAMPP_LIN_SERIES_BELOW)
		return 1.0 / 12 + t2 * (1.0 / 720 + t2 * (1.0 / 30240 + t2 * (1.0 / 1209600)));
	const double f_half = .5 * f_theta;
	return 1 / t2 - cos(f_half) / (2 * f_theta * sin(f_half));
}

// M (column-major 3 x 3) = I + f_half_sign / 2 [phi]x + c(|phi|) [phi]x^2: f_half_sign = -1 the inverse of the left Jacobian
// of SO(3) at phi, +1 that of the right one
SLAMPP_LIN_FN void inv_jacobian(const double *phi, double f_half_sign, double *M)
{
	const double x = phi[0], y = phi[1], z = phi[2], t2 = x * x + y * y + z * z;
	const double c = inv_jacobian_c(sqrt(t2)), h = .5 * f_half_sign;
	M[0] = 1 + c * (x * x - t2); M[3] = c * x * y - h * z;    M[6] = c * x * z + h * y;
	M[1] = c * x * y + h * z;    M[4] = 1 + c * (y * y - t2); M[7] = c * y * z - h * x;
	M[2] = c * x * z - h * y;    M[5] = c * y * z + h * x;    M[8] = 1 + c * (z * z - t2);
}

// ---- the edges: x0, x1 the states of the two vertices, z the measurement; J0 (RD x D0), J1 (RD x D1) column-major ----

SLAMPP_LIN_FN void edge_se2(const double *x0, const double *x1, const double *z, double *J0, double *J1, double *err)
{
	const double c = cos(x0[2]), s = sin(x0[2]), de = x1[0] - x0[0], dn = x1[1] - x0[1];
	const double h0 = c * de + s * dn, h1 = c * dn - s * de, h2 = clamp_angle_2pi(x1[2] - x0[2]);
	err[0] = z[0] - h0;
	err[1] = z[1] - h1;
	err[2] = clamp_angular_error_2pi(z[2] - h2);
	J0[0] = -c; J0[3] = -s; J0[6] = h1;
	J0[1] = s;  J0[4] = -c; J0[7] = -h0;
	J0[2] = 0;  J0[5] = 0;  J0[8] = -1;
	J1[0] = c;  J1[3] = s;  J1[6] = 0;
	J1[1] = -s; J1[4] = c;  J1[7] = 0;
	J1[2] = 0;  J1[5] = 0;  J1[8] = 1;
}

SLAMPP_LIN_FN void edge_se3(const double *x0, const double *x1, const double *z, double *J0, double *J1, double *err)
{
	const TQuat q0 = quat_exp(x0 + 3);
	TQuat qd = quat_mul(quat_conj(q0), quat_exp(x1 + 3));
	if(qd.w < 0) {
		qd.w = -qd.w; qd.x = -qd.x; qd.y = -qd.y; qd.z = -qd.z;
	}
	double R0[9], Rd[9], ht[3], hr[3], M[9];
	quat_to_rot(q0, R0);
	quat_to_rot(qd, Rd);
	quat_log(qd, hr);
	const double dt[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]};
	#pragma unroll
	for(int i = 0; i < 3; ++ i) {
		ht[i] = R0[3 * i] * dt[0] + R0[3 * i + 1] * dt[1] + R0[3 * i + 2] * dt[2]; // (row i of R0^T)
		err[i] = z[i] - ht[i];
	}
	quat_log(quat_mul(quat_exp(z + 3), quat_conj(qd)), err + 3);
	#pragma unroll
	for(int i = 0; i < 36; ++ i)
		J0[i] = J1[i] = 0;
	J0[0] = J0[7] = J0[14] = -1;
	J0[6 * 3 + 0] = 0;      J0[6 * 4 + 0] = -ht[2]; J0[6 * 5 + 0] = ht[1]; // [h_t]x
	J0[6 * 3 + 1] = ht[2];  J0[6 * 4 + 1] = 0;      J0[6 * 5 + 1] = -ht[0];
	J0[6 * 3 + 2] = -ht[1]; J0[6 * 4 + 2] = ht[0];  J0[6 * 5 + 2] = 0;
	inv_jacobian(hr, -1, M);
	#pragma unroll
	for(int c = 0; c < 3; ++ c) {
		#pragma unroll
		for(int r = 0; r < 3; ++ r)
			J0[6 * (3 + c) + 3 + r] = -M[3 * c + r];
	}
	inv_jacobian(hr, 1, M);
	#pragma unroll
	for(int c = 0; c < 3; ++ c) {
		#pragma unroll
		for(int r = 0; r < 3; ++ r) {
			J1[6 * c + r] = Rd[3 * c + r];
			J1[6 * (3 + c) + 3 + r] = M[3 * c + r];
		}
	}
}

// x0 the camera (t, axis-angle), x1 the point, k5 the camera's intrinsics (fx, fy, cx, cy, k)
SLAMPP_LIN_FN void edge_p2c_xyz(const double *x0, const double *x1, const double *z, const double *k5, double *J0, double *J1,
	double *err)
{
	double R[9];
	quat_to_rot(quat_exp(x0 + 3), R);
	const double X = x1[0], Y = x1[1], Z = x1[2];
	const double cx = R[0] * X + R[3] * Y + R[6] * Z + x0[0], cy = R[1] * X + R[4] * Y + R[7] * Z + x0[1],
		cz = R[2] * X + R[5] * Y + R[8] * Z + x0[2];
	const double fx = k5[0], fy = k5[1], k = k5[4] / (.5 * (fx + fy)), iz = 1 / cz;
	const double px = fx * cx * iz, py = fy * cy * iz, g = 1 + k * (px * px + py * py);
	err[0] = z[0] - (k5[2] + g * px);
	err[1] = z[1] - (k5[3] + g * py);
	// D = d projection / d x (2 x 3) = [g I + 2 k p p^T] [fx / z, 0, -px / z; 0, fy / z, -py / z]
	const double a00 = g + 2 * k * px * px, a01 = 2 * k * px * py, a11 = g + 2 * k * py * py;
	const double b00 = fx * iz, b02 = -px * iz, b11 = fy * iz, b12 = -py * iz;
	const double D[6] = {a00 * b00, a01 * b00, a01 * b11, a11 * b11, a00 * b02 + a01 * b12, a01 * b02 + a11 * b12}; // column-major
	#pragma unroll
	for(int c = 0; c < 3; ++ c) {
		#pragma unroll
		for(int r = 0; r < 2; ++ r)
			J1[2 * c + r] = J0[2 * c + r] = D[r] * R[3 * c] + D[2 + r] * R[3 * c + 1] + D[4 + r] * R[3 * c + 2]; // D R
	}
	#pragma unroll
	for(int r = 0; r < 2; ++ r) { // -D R [X]x
		J0[6 + r] = J1[4 + r] * Y - J1[2 + r] * Z;
		J0[8 + r] = J1[r] * Z - J1[4 + r] * X;
		J0[10 + r] = J1[2 + r] * X - J1[r] * Y;
	}
}

// x0 the pose (e, n, theta), x1 the landmark (e, n), z = (range, bearing).  A range below 1e-5 is replaced by 1e-5 in the
// expectation and in the denominators of both Jacobians, as the reference does (2DSolverBase.h:475-495); the numerators keep
// the true differences.  The operations are the reference's, in its order: a host build without contraction gives its bits.
SLAMPP_LIN_FN void edge_pose_landmark_2d(const double *x0, const double *x1, const double *z, double *J0, double *J1, double *err)
{
	const double de = x1[0] - x0[0], dn = x1[1] - x0[1];
	double r = sqrt(de * de + dn * dn);
	const double b = clamp_angle_2pi(atan2(dn, de) - x0[2]);
	if(fabs(r) < 1e-5)
		r = 1e-5;
	const double r2 = r * r;
	err[0] = z[0] - r;
	err[1] = clamp_angular_error_2pi(z[1] - b);
	J0[0] = -de / r; J0[2] = -dn / r;  J0[4] = 0;
	J0[1] = dn / r2; J0[3] = -de / r2; J0[5] = -1;
	J1[0] = de / r;   J1[2] = dn / r;
	J1[1] = -dn / r2; J1[3] = de / r2;
}

// x0 the pose (t, axis-angle), x1 the landmark, z the landmark in the pose's frame: h = R0^T (X - t0), J0 = [-I, [h]x]
// (the SE(3) (+) of edge_se3), J1 = R0^T
SLAMPP_LIN_FN void edge_pose_landmark_3d(const double *x0, const double *x1, const double *z, double *J0, double *J1, double *err)
{
	double R[9], h[3];
	quat_to_rot(quat_exp(x0 + 3), R);
	const double dt[3] = {x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]};
	#pragma unroll
	for(int i = 0; i < 3; ++ i) {
		h[i] = R[3 * i] * dt[0] + R[3 * i + 1] * dt[1] + R[3 * i + 2] * dt[2]; // (row i of R0^T)
		err[i] = z[i] - h[i];
	}
	#pragma unroll
	for(int i = 0; i < 9; ++ i)
		J0[i] = 0;
	J0[0] = J0[4] = J0[8] = -1;
	J0[9] = 0;      J0[12] = -h[2]; J0[15] = h[1]; // [h]x
	J0[10] = h[2];  J0[13] = 0;     J0[16] = -h[0];
	J0[11] = -h[1]; J0[14] = h[0];  J0[17] = 0;
	#pragma unroll
	for(int c = 0; c < 3; ++ c) {
		#pragma unroll
		for(int r = 0; r < 3; ++ r)
			J1[3 * c + r] = R[3 * r + c];
	}
}

// x0 the camera (t, axis-angle), x1 the point, k6 the stereo camera's (fx, fy, cx, cy, k, baseline); z = (u, v) in the left
// image and u in the right one.  Each image is p = (fx x / z, fy y / z), projection = c + (1 + k' |p|) p with
// k' = k / ((fx + fy) / 2): the radial term is linear in |p| here (BASolverBase.h:516-517, 530-531), where the monocular
// edge has |p|^2.  The right image sees the camera-frame point moved by -baseline along x.  With A = d projection / dp
// = (1 + k' |p|) I + k' p p^T / |p| (I at p = 0), D (3 x 3) = d (u, v, u_right) / d x stacks the two rows of the left image's
// A [fx / z, 0, -px / z; 0, fy / z, -py / z] on the first row of the right one's; then as edge_p2c_xyz.
SLAMPP_LIN_FN void edge_p2sc_xyz(const double *x0, const double *x1, const double *z, const double *k6, double *J0, double *J1,
	double *err)
{
	double R[9];
	quat_to_rot(quat_exp(x0 + 3), R);
	const double X = x1[0], Y = x1[1], Z = x1[2];
	const double cx = R[0] * X + R[3] * Y + R[6] * Z + x0[0], cy = R[1] * X + R[4] * Y + R[7] * Z + x0[1],
		cz = R[2] * X + R[5] * Y + R[8] * Z + x0[2];
	const double fx = k6[0], fy = k6[1], k = k6[4] / (.5 * (fx + fy)), iz = 1 / cz;
	const double px = fx * cx * iz, py = fy * cy * iz, qx = fx * (cx - k6[5]) * iz;
	const double rl = sqrt(px * px + py * py), rr = sqrt(qx * qx + py * py), gl = 1 + k * rl, gr = 1 + k * rr;
	err[0] = z[0] - (k6[2] + gl * px);
	err[1] = z[1] - (k6[3] + gl * py);
	err[2] = z[2] - (k6[2] + gr * qx);
	const double kl = (rl > 0)? k / rl : 0, kr = (rr > 0)? k / rr : 0;
	const double a00 = gl + kl * px * px, a01 = kl * px * py, a11 = gl + kl * py * py, c00 = gr + kr * qx * qx, c01 = kr * qx * py;
	const double b00 = fx * iz, b02 = -px * iz, b11 = fy * iz, b12 = -py * iz, e02 = -qx * iz;
	const double D[9] = {a00 * b00, a01 * b00, c00 * b00, a01 * b11, a11 * b11, c01 * b11, a00 * b02 + a01 * b12, a01 * b02 + a11 * b12,
		c00 * e02 + c01 * b12}; // column-major
	#pragma unroll
	for(int c = 0; c < 3; ++ c) {
		#pragma unroll
		for(int r = 0; r < 3; ++ r)
			J1[3 * c + r] = J0[3 * c + r] = D[r] * R[3 * c] + D[3 + r] * R[3 * c + 1] + D[6 + r] * R[3 * c + 2]; // D R
	}
	#pragma unroll
	for(int r = 0; r < 3; ++ r) { // -D R [X]x
		J0[9 + r] = J1[6 + r] * Y - J1[3 + r] * Z;
		J0[12 + r] = J1[r] * Z - J1[6 + r] * X;
		J0[15 + r] = J1[3 + r] * X - J1[r] * Y;
	}
}

// ---- the vertices: out = x (+) s dx; out may be x ----

SLAMPP_LIN_FN void plus_se2(const double *x, const double *dx, double s, double *out)
{
	const double a = x[0] + s * dx[0], b = x[1] + s * dx[1], t = x[2] + s * dx[2];
	out[0] = a; out[1] = b;
	out[2] = clamp_angle_2pi(t);
}

SLAMPP_LIN_FN void plus_se3(const double *x, const double *dx, double s, double *out)
{
	const double e[6] = {s * dx[0], s * dx[1], s * dx[2], s * dx[3], s * dx[4], s * dx[5]};
	const TQuat q = quat_exp(x + 3);
	double R[9], r[3];
	quat_to_rot(q, R);
	quat_log(quat_mul(q, quat_exp(e + 3)), r);
	const double t0 = x[0] + R[0] * e[0] + R[3] * e[1] + R[6] * e[2], t1 = x[1] + R[1] * e[0] + R[4] * e[1] + R[7] * e[2],
		t2 = x[2] + R[2] * e[0] + R[5] * e[1] + R[8] * e[2];
	out[0] = t0; out[1] = t1; out[2] = t2;
	out[3] = r[0]; out[4] = r[1]; out[5] = r[2];
}

} // namespace lin
} // namespace slampp
