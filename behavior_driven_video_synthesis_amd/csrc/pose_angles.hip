// The angle-space pose path (keypoint_type ``angle_world_expmap``): forward kinematics, the root's path and the Euler-angle
// error.  Interface: include/vunet_pose_angles.h.
//
// The reference does all three on the host, frame by frame and joint by joint (data/data_conversions_3d.py:608-703, :1047-1066;
// lib/metrics.py:321-357; fkl builds one dict per joint per frame).  Here:
//   * pose_fk_kernel: one lane per pose walks the tree in index order.  The per-joint rotations and positions the children read
//     back sit in the lane's private memory (12 doubles a joint): the launch is a few thousand poses of 32 joints, nothing in it is
//     worth a layout of its own.
//   * pose_revert_root_kernel: a scan over the frames, one lane per sequence; the block first copies the dimensions it leaves alone.
//   * pose_euler_error_kernel: one workgroup per sequence.  gt's Euler angles sit in LDS ([T][D] doubles); the kept-dimension mask
//     comes from them, then the squared differences to rec's angles overwrite them in place, then per-frame norms and the horizon
//     means, every sum in index order.
// Everything is float64 with one rounding on the fp32 store; no atomics, no hand-off between workgroups.
#include "common.h"
#include "../../include/vunet_pose_angles.h"

namespace {

#define POSE_EPS32 1.1920928955078125e-07   // np.finfo(np.float32).eps, the reference's guard in three divisions
#define POSE_PI 3.141592653589793
#define POSE_2PI 6.283185307179586

// unNormalizeData (data/data_conversions_3d.py:178-211) of dimension d: pos_of_dim[d] is its column among the used ones, -1 for an
// ignored dimension (0 * std + mean).  numpy's promotion: float32 statistics keep x * std + mean in float32, two roundings, no
// fused multiply-add.
__device__ __forceinline__ double pose_dim(const float* __restrict__ row, const int* __restrict__ pos_of_dim, const double* __restrict__ mean,
                                           const double* __restrict__ stdv, int f32, int d) {
#pragma clang fp contract(off)
  const int p = pos_of_dim[d];
  const float v = p >= 0 ? row[p] : 0.f;
  if (f32) return (double)(v * (float)stdv[d] + (float)mean[d]);
  return (double)v * stdv[d] + mean[d];
}

__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt((a * a + b * b) + c * c); }

// expmap2rotmat (:154-175): Rodrigues' formula with the axis r / (|r| + eps); R row-major
__device__ __forceinline__ void expmap_to_rotmat(double rx, double ry, double rz, double* __restrict__ R) {
  const double theta = norm3(rx, ry, rz);
  const double den = theta + POSE_EPS32;
  const double x = rx / den, y = ry / den, z = rz / den;
  const double s = sin(theta), c1 = 1.0 - cos(theta);
  // K = [[0, -z, y], [z, 0, -x], [-y, x, 0]];  K K = [[-(y y + z z), x y, x z], [x y, -(x x + z z), y z], [x z, y z, -(x x + y y)]]
  R[0] = 1.0 + c1 * (-(z * z) - y * y);
  R[1] = s * -z + c1 * (y * x);
  R[2] = s * y + c1 * (z * x);
  R[3] = s * z + c1 * (x * y);
  R[4] = 1.0 + c1 * (-(z * z) - x * x);
  R[5] = s * -x + c1 * (z * y);
  R[6] = s * -y + c1 * (x * z);
  R[7] = s * x + c1 * (y * z);
  R[8] = 1.0 + c1 * (-(y * y) - x * x);
}

// C = A . B, 3x3 row-major
__device__ __forceinline__ void matmul3(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// rotmat2euler (:56-85), the R[0][2] == +-1 branch as written (E3 = 0)
__device__ __forceinline__ void rotmat_to_euler(const double* __restrict__ R, double* __restrict__ e) {
  if (R[2] == 1.0 || R[2] == -1.0) {
    const double dlta = atan2(R[1], R[2]);
    e[0] = dlta;
    e[1] = R[2] == -1.0 ? POSE_PI / 2 : -POSE_PI / 2;
    e[2] = 0.0;
  } else {
    const double e2 = -asin(R[2]), c = cos(e2);
    e[0] = atan2(R[5] / c, R[8] / c);
    e[1] = e2;
    e[2] = atan2(R[1] / c, R[0] / c);
  }
}

// quat2expmap(rotmat2quat(R)) (:88-151); the reference's print on a non-unit quaternion is not reproduced
__device__ __forceinline__ void rotmat_to_expmap(const double* __restrict__ R, double* __restrict__ r) {
  // rotmat2quat: the axis from R - R^T, the angle from its norm and the trace
  const double ax = -(R[5] - R[7]), ay = R[2] - R[6], az = -(R[1] - R[3]);
  const double an = norm3(ax, ay, az);
  const double sintheta = an / 2, costheta = (((R[0] + R[4]) + R[8]) - 1.0) / 2;
  const double half = atan2(sintheta, costheta) / 2;
  const double q0 = cos(half), sh = sin(half), dq = an + POSE_EPS32;
  const double q1 = ax / dq * sh, q2 = ay / dq * sh, q3 = az / dq * sh;
  // quat2expmap
  const double qn = norm3(q1, q2, q3), de = qn + POSE_EPS32;
  double x = q1 / de, y = q2 / de, z = q3 / de;
  double theta = 2 * atan2(qn, q0);
  theta = fmod(theta + POSE_2PI, POSE_2PI);
  if (theta > POSE_PI) {
    theta = POSE_2PI - theta;
    x = -x;
    y = -y;
    z = -z;
  }
  r[0] = x * theta;
  r[1] = y * theta;
  r[2] = z * theta;
}

__global__ __launch_bounds__(64) void pose_fk_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ pos_of_dim,
                                                     const double* __restrict__ mean, const double* __restrict__ stdv, int f32, int D,
                                                     const int* __restrict__ parent, const double* __restrict__ offset,
                                                     const int* __restrict__ expmap_ind, const int* __restrict__ pos_ind, int J, int swap_yz,
                                                     float* __restrict__ xyz, int T) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  const float* row = x + (size_t)t * ldx;
  auto dim = [&](int d) -> double { return pos_of_dim ? pose_dim(row, pos_of_dim, mean, stdv, f32, d) : (double)row[d]; };
  double rot[VUNET_POSE_MAX_JOINTS][9], pos[VUNET_POSE_MAX_JOINTS][3];
  float* out = xyz + (size_t)t * J * 3;
  const int iy = swap_yz ? 2 : 1, iz = swap_yz ? 1 : 2;
  for (int j = 0; j < J; ++j) {
    double R[9];
    expmap_to_rotmat(dim(expmap_ind[3 * j]), dim(expmap_ind[3 * j + 1]), dim(expmap_ind[3 * j + 2]), R);
    const double ox = offset[3 * j], oy = offset[3 * j + 1], oz = offset[3 * j + 2];
    const int p = parent[j];
    if (p < 0) {   // a root: offset + translation, its own rotation
      pos[j][0] = ox + (pos_ind ? dim(pos_ind[0]) : 0.0);
      pos[j][1] = oy + (pos_ind ? dim(pos_ind[1]) : 0.0);
      pos[j][2] = oz + (pos_ind ? dim(pos_ind[2]) : 0.0);
#pragma unroll
      for (int k = 0; k < 9; ++k) rot[j][k] = R[k];
    } else {       // offset . R_parent + xyz_parent;  R_this . R_parent
      const double* Rp = rot[p];
#pragma unroll
      for (int c = 0; c < 3; ++c) pos[j][c] = ((ox * Rp[c] + oy * Rp[3 + c]) + oz * Rp[6 + c]) + pos[p][c];
      matmul3(R, Rp, rot[j]);
    }
    out[3 * j] = (float)pos[j][0];
    out[3 * j + iy] = (float)pos[j][1];
    out[3 * j + iz] = (float)pos[j][2];
  }
}

__global__ __launch_bounds__(64) void pose_revert_root_kernel(const float* __restrict__ ch, const double* __restrict__ r0,
                                                              const double* __restrict__ t0, float* __restrict__ out, int B, int T, int D) {
  const int b0 = blockIdx.x * 64, nb = min(64, B - b0);
  // the dimensions the scan does not touch: the block's sequences are contiguous rows of D
  const size_t base = (size_t)b0 * T * D, rows = (size_t)nb * T;
  for (size_t k = threadIdx.x; k < rows * (D - 6); k += 64) {
    const size_t r = k / (D - 6), d = 6 + (k - r * (D - 6));
    out[base + r * D + d] = ch[base + r * D + d];
  }
  if ((int)threadIdx.x >= nb) return;
  const size_t seq = base + (size_t)threadIdx.x * T * D;
  double Rp[9], Tp[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rp[k] = r0[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) Tp[k] = t0[k];
  for (int t = 0; t < T; ++t) {
    const float* c = ch + seq + (size_t)t * D;
    float* o = out + seq + (size_t)t * D;
    const double tx = c[0], ty = c[1], tz = c[2];
    double Rd[9], R[9], r[3];
    expmap_to_rotmat((double)c[3], (double)c[4], (double)c[5], Rd);
    matmul3(Rd, Rp, R);
    rotmat_to_expmap(R, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // T_prev + R_prev^T . translation
      Tp[k] = Tp[k] + ((Rp[k] * tx + Rp[3 + k] * ty) + Rp[6 + k] * tz);
      o[k] = (float)Tp[k];
      o[3 + k] = (float)r[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Rp[k] = R[k];
  }
}

// the Euler angles of triple k of one un-normalised frame (k == 0: the translation, left as it is)
__device__ __forceinline__ void frame_triple(const float* __restrict__ row, const int* __restrict__ pos_of_dim,
                                             const double* __restrict__ mean, const double* __restrict__ stdv, int f32, int k,
                                             double* __restrict__ e) {
  const double a = pose_dim(row, pos_of_dim, mean, stdv, f32, 3 * k), b = pose_dim(row, pos_of_dim, mean, stdv, f32, 3 * k + 1),
               c = pose_dim(row, pos_of_dim, mean, stdv, f32, 3 * k + 2);
  if (k == 0) {
    e[0] = a;
    e[1] = b;
    e[2] = c;
    return;
  }
  double R[9];
  expmap_to_rotmat(a, b, c, R);
  rotmat_to_euler(R, e);
}

__global__ __launch_bounds__(256) void pose_euler_error_kernel(const float* __restrict__ rec, const float* __restrict__ gt, int n_use,
                                                               const int* __restrict__ pos_of_dim, const double* __restrict__ mean,
                                                               const double* __restrict__ stdv, int f32, int D,
                                                               const int* __restrict__ horizons, int n_h, float* __restrict__ out, int T) {
  extern __shared__ double lds[];
  double* G = lds;                              // [T][D]: gt's Euler angles, later the kept squared differences
  double* fnorm = lds + (size_t)T * D;          // [T]: per-frame norms
  int* keep = reinterpret_cast<int*>(fnorm + T);   // [D]
  const int b = blockIdx.x, K = D / 3;
  const float* rb = rec + (size_t)b * T * n_use;
  const float* gb = gt + (size_t)b * T * n_use;
  for (int i = threadIdx.x; i < T * K; i += 256) {
    const int t = i / K, k = i - t * K;
    double e[3] = {0.0, 0.0, 0.0};              // the global translation and rotation of gt are set to 0
    if (k >= 2) frame_triple(gb + (size_t)t * n_use, pos_of_dim, mean, stdv, f32, k, e);
    G[t * D + 3 * k] = e[0];
    G[t * D + 3 * k + 1] = e[1];
    G[t * D + 3 * k + 2] = e[2];
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {  // np.std(gt, 0) > 1e-4: the population deviation over the T frames
    double m = 0.0, v = 0.0;
    for (int t = 0; t < T; ++t) m += G[t * D + d];
    m /= (double)T;
    for (int t = 0; t < T; ++t) {
      const double c = G[t * D + d] - m;
      v += c * c;
    }
    keep[d] = sqrt(v / (double)T) > 1e-4 ? 1 : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * K; i += 256) {
    const int t = i / K, k = i - t * K;
    double e[3];
    frame_triple(rb + (size_t)t * n_use, pos_of_dim, mean, stdv, f32, k, e);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int d = 3 * k + a;
      const double c = G[t * D + d] - e[a];
      G[t * D + d] = keep[d] ? c * c : 0.0;
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < T; t += 256) {
    double s = 0.0;
    for (int d = 0; d < D; ++d)
      if (keep[d]) s += G[t * D + d];
    fnorm[t] = sqrt(s);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < n_h; h += 256) {   // the numpy slice [:e] of T frames holds min(e, T) of them
    const int m = min(horizons[h], T);
    double s = 0.0;
    for (int t = 0; t < m; ++t) s += fnorm[t];
    out[(size_t)b * n_h + h] = (float)(s / (double)m);
  }
}

}  // namespace

extern "C" int vunet_pose_fk(const float* x, int32_t ldx, const int32_t* pos_of_dim, const double* mean, const double* stdv,
                             int32_t f32_math, int32_t D, const int32_t* parent, const double* offset, const int32_t* expmap_ind,
                             const int32_t* pos_ind, int32_t J, int32_t swap_yz, float* xyz, int32_t T, void* stream) {
  if (!x || !parent || !offset || !expmap_ind || !xyz || T < 1 || D < 3 || ldx < 1 || J < 1 || J > VUNET_POSE_MAX_JOINTS)
    return VUNET_ERR_ARG;
  if (pos_of_dim ? (!mean || !stdv || ldx > D) : ldx < D) return VUNET_ERR_ARG;
  VUNET_LAUNCH(pose_fk_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, (hipStream_t)stream, x, ldx, pos_of_dim, mean, stdv,
               f32_math ? 1 : 0, D, parent, offset, expmap_ind, pos_ind, J, swap_yz ? 1 : 0, xyz, T);
  return vunet_check_launch();
}

extern "C" int vunet_pose_revert_root(const float* ch, const double* r0, const double* t0, float* out, int32_t B, int32_t T, int32_t D,
                                      void* stream) {
  if (!ch || !r0 || !t0 || !out || B < 1 || T < 1 || D < 6) return VUNET_ERR_ARG;
  VUNET_LAUNCH(pose_revert_root_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, ch, r0, t0, out, B, T, D);
  return vunet_check_launch();
}

extern "C" int vunet_pose_euler_error(const float* rec, const float* gt, int32_t n_use, const int32_t* pos_of_dim, const double* mean,
                                      const double* stdv, int32_t f32_math, int32_t D, const int32_t* horizons, int32_t n_h, float* out,
                                      int32_t B, int32_t T, void* stream) {
  if (!rec || !gt || !pos_of_dim || !mean || !stdv || !horizons || !out || B < 1 || T < 1 || n_use < 1 || n_use > D || D < 6 || D % 3 ||
      n_h < 1 || n_h > 256)
    return VUNET_ERR_ARG;
  if (D > VUNET_POSE_EULER_MAX_D || (int64_t)T * (D + 1) > VUNET_POSE_EULER_MAX_TD) return VUNET_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)T * D + T) * sizeof(double) + (size_t)D * sizeof(int);
  VUNET_LAUNCH(pose_euler_error_kernel, dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream, rec, gt, n_use, pos_of_dim, mean, stdv,
               f32_math ? 1 : 0, D, horizons, n_h, out, T);
  return vunet_check_launch();
}
