// Geometry set-up of the hexahedral operators (a2/a13): per-point G and det J w of trilinear cells, written in the
// blocked symmetric layout that the stiffness kernels stream, for dofmap meshes, slot lists and structured boxes.
#include "common.h"

namespace wf {

__device__ __forceinline__ double clamp101(double v)
{
  // xt::isclose(v, b) with rtol 1e-5, atol 1e-8, applied for b = -1, 0, 1
  // (common/precomputation.hpp:105-107)
  if (fabs(v + 1.0) <= 1e-8 + 1e-5) v = -1.0;
  if (fabs(v) <= 1e-8) v = 0.0;
  if (fabs(v - 1.0) <= 1e-8 + 1e-5) v = 1.0;
  return v;
}

__device__ __forceinline__ double det3(const double* A)
{
  return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])
         + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// Jacobian, |det J| w and G = (J^-1 detJ) J^-T at one point of a trilinear
// hexahedron (common/precomputation.hpp:83-100).  xv: the cell's 8 vertices
// [v][3], vertex v = a + 2b + 4c; X: reference point.
__device__ __forceinline__ void hex_point_geometry(const double (*xv)[3], double X0, double X1, double X2,
                                                   double w, int use_fabs, int do_clamp, double* G9,
                                                   double* detJw)
{
  double J[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) J[i] = 0.0;
  const double f0[2] = {1.0 - X0, X0}, f1[2] = {1.0 - X1, X1}, f2[2] = {1.0 - X2, X2};
  const double g[2] = {-1.0, 1.0};
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const int a = v & 1, b = (v >> 1) & 1, c = (v >> 2) & 1;
    // the reference clamps the tabulated cmap derivatives to -1/0/1
    // (precomputation.hpp:56-58)
    double d0 = g[a] * f1[b] * f2[c];
    double d1 = f0[a] * g[b] * f2[c];
    double d2 = f0[a] * f1[b] * g[c];
    if (do_clamp) {
      d0 = clamp101(d0);
      d1 = clamp101(d1);
      d2 = clamp101(d2);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      J[i * 3 + 0] += xv[v][i] * d0;
      J[i * 3 + 1] += xv[v][i] * d1;
      J[i * 3 + 2] += xv[v][i] * d2;
    }
  }
  double d = det3(J);
  const double idet = 1.0 / d;
  if (use_fabs) d = fabs(d);
  d *= w;
  *detJw = d;
  if (G9) {
    double Ji[9];
    Ji[0] = (J[4] * J[8] - J[5] * J[7]) * idet;
    Ji[1] = (J[2] * J[7] - J[1] * J[8]) * idet;
    Ji[2] = (J[1] * J[5] - J[2] * J[4]) * idet;
    Ji[3] = (J[5] * J[6] - J[3] * J[8]) * idet;
    Ji[4] = (J[0] * J[8] - J[2] * J[6]) * idet;
    Ji[5] = (J[2] * J[3] - J[0] * J[5]) * idet;
    Ji[6] = (J[3] * J[7] - J[4] * J[6]) * idet;
    Ji[7] = (J[1] * J[6] - J[0] * J[7]) * idet;
    Ji[8] = (J[0] * J[4] - J[1] * J[3]) * idet;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) s += (Ji[i * 3 + k] * d) * Ji[j * 3 + k];
        G9[i * 3 + j] = do_clamp ? clamp101(s) : s;
      }
  }
}

// Cell coefficient a_c (wavehip.h, "Cell coefficients"): the finished entries of a point -- G after the clamp, det J w --
// times a_c, one rounding each.  The geometry kernels call it only when the operator has a coefficient array; c is
// the kernel's own cell index, so the array comes in the order of the cells the kernel is given.
__device__ __forceinline__ void scale_point_geometry(double a, double* G9, double* detJw)
{
  *detJw *= a;
  if (G9) {
#pragma unroll
    for (int m = 0; m < 9; ++m) G9[m] *= a;
  }
}

// Blocked symmetric geometry layout shared by the stiffness kernels:
//   G6blk[batch][k][p][t][e],  t = cl * n^2 + (j * n + i) < NT = CB * n^2,
//   (p, e) -> component: (0,0)=G00 (0,1)=G01 (1,0)=G02 (1,1)=G11 (2,0)=G12 (2,1)=G22
__device__ __forceinline__ size_t g6_index(int n, int NT, size_t batch, int k, int p, int t, int e)
{
  return ((((batch * n + k) * 3 + p) * (size_t)NT + t) * 2) + e;
}

__device__ __forceinline__ void store_g6(double* G6blk, int n, int NT, size_t batch, int k, int t,
                                         const double* G9)
{
  G6blk[g6_index(n, NT, batch, k, 0, t, 0)] = G9[0];
  G6blk[g6_index(n, NT, batch, k, 0, t, 1)] = G9[1];
  G6blk[g6_index(n, NT, batch, k, 1, t, 0)] = G9[2];
  G6blk[g6_index(n, NT, batch, k, 1, t, 1)] = G9[4];
  G6blk[g6_index(n, NT, batch, k, 2, t, 0)] = G9[5];
  G6blk[g6_index(n, NT, batch, k, 2, t, 1)] = G9[8];
}

// --------------------------------------------------------------------------
// geometry kernels (setup; a2/a13)
// --------------------------------------------------------------------------
__global__ void k_geometry_hex(int n, int CB, int ncells, const double* __restrict__ xverts,
                               const int32_t* __restrict__ geom_dofmap, const double* __restrict__ pts,
                               const double* __restrict__ wts, int use_fabs, int do_clamp,
                               double* __restrict__ G9out, double* __restrict__ G6blk,
                               double* __restrict__ detJ, const double* __restrict__ cell_coeff)
{
  const int nd = n * n * n;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)ncells * nd) return;
  const int c = (int)(gid / nd), q = (int)(gid % nd);
  const int i = q % n, j = (q / n) % n, k = q / (n * n);
  double xv[8][3];
  for (int v = 0; v < 8; ++v) {
    const int32_t vi = geom_dofmap[(size_t)c * 8 + v];
    xv[v][0] = xverts[(size_t)vi * 3 + 0];
    xv[v][1] = xverts[(size_t)vi * 3 + 1];
    xv[v][2] = xverts[(size_t)vi * 3 + 2];
  }
  double G9[9], d;
  const bool wantG = (G9out != nullptr) || (G6blk != nullptr);
  hex_point_geometry(xv, pts[i], pts[j], pts[k], wts[i] * wts[j] * wts[k], use_fabs, do_clamp,
                     wantG ? G9 : nullptr, &d);
  if (cell_coeff) scale_point_geometry(cell_coeff[c], wantG ? G9 : nullptr, &d);
  if (detJ) detJ[gid] = d;
  if (G9out)
    for (int m = 0; m < 9; ++m) G9out[gid * 9 + m] = G9[m];
  if (G6blk) {
    const int NT = CB * n * n;
    store_g6(G6blk, n, NT, c / CB, k, (c % CB) * n * n + j * n + i, G9);
  }
}

// the same for a subset of slots of the blocked layout: cell c of the list goes to slot slot_of[c]
// (batch = slot / CB); used by the indexed marching operator, whose slot array has gaps
// cell_sign (may be null): -1 for cells whose vertices were handed over in a reflected frame (lattice
// plan, generic_plan.cpp).  G = K K^T |det J| w does not depend on the frame; without the fabs
// (spectral_mass.hpp:58-64) det J changes sign under a reflection and is corrected here.
__global__ void k_geometry_hex_slots(int n, int CB, int ncells, const double* __restrict__ xverts,
                                     const int32_t* __restrict__ geom_dofmap, const int32_t* __restrict__ slot_of,
                                     const int8_t* __restrict__ cell_sign,
                                     const double* __restrict__ pts, const double* __restrict__ wts, int use_fabs,
                                     int do_clamp, double* __restrict__ G6blk, const double* __restrict__ cell_coeff)
{
  const int nd = n * n * n;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)ncells * nd) return;
  const int c = (int)(gid / nd), q = (int)(gid % nd);
  const int i = q % n, j = (q / n) % n, k = q / (n * n);
  double xv[8][3];
  for (int v = 0; v < 8; ++v) {
    const int32_t vi = geom_dofmap[(size_t)c * 8 + v];
    xv[v][0] = xverts[(size_t)vi * 3 + 0];
    xv[v][1] = xverts[(size_t)vi * 3 + 1];
    xv[v][2] = xverts[(size_t)vi * 3 + 2];
  }
  double G9[9], d;
  hex_point_geometry(xv, pts[i], pts[j], pts[k], wts[i] * wts[j] * wts[k], use_fabs, do_clamp, G9, &d);
  if (!use_fabs && cell_sign && cell_sign[c] < 0)
    for (int m = 0; m < 9; ++m) G9[m] = -G9[m];
  if (cell_coeff) scale_point_geometry(cell_coeff[c], G9, &d);
  const int slot = slot_of[c];
  store_g6(G6blk, n, CB * n * n, slot / CB, k, (slot % CB) * n * n + j * n + i, G9);
}

// reference-layout G[ncells][nq][3][3] -> blocked symmetric layout (upper triangle)
__global__ void k_pack_G6(int n, int CB, int ncells, const double* __restrict__ G9in,
                          double* __restrict__ G6blk)
{
  const int nd = n * n * n;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)ncells * nd) return;
  const int c = (int)(gid / nd), q = (int)(gid % nd);
  const int i = q % n, j = (q / n) % n, k = q / (n * n);
  double G9[9];
  for (int m = 0; m < 9; ++m) G9[m] = G9in[gid * 9 + m];
  store_g6(G6blk, n, CB * n * n, c / CB, k, (c % CB) * n * n + j * n + i, G9);
}

// Structured box: one thread per (cell, point); the cell's vertices come from the
// vertex lattice.  Writes the blocked G of the box stiffness kernel (block =
// bx*by*bz cells, padded blocks stay zero) and/or accumulates the lumped mass
// diagonal m[g] += |det J| w on the dof lattice.
__global__ void k_geometry_box(int n, int nx, int ny, int nz, int bx, int by, int bz,
                               const double* __restrict__ xverts, const double* __restrict__ pts,
                               const double* __restrict__ wts, int use_fabs, int do_clamp,
                               double* __restrict__ G6blk, double* __restrict__ mdiag,
                               const double* __restrict__ cell_coeff)
{
  const int P = n - 1, nd = n * n * n;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t ncells = (size_t)nx * ny * nz;
  if (gid >= ncells * nd) return;
  const int c = (int)(gid / nd), q = (int)(gid % nd);
  const int i = q % n, j = (q / n) % n, k = q / (n * n);
  const int cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
  double xv[8][3];
  for (int v = 0; v < 8; ++v) {
    const size_t vi = (size_t)(cx + (v & 1)) + (size_t)(nx + 1) * ((cy + ((v >> 1) & 1)) + (size_t)(ny + 1) * (cz + ((v >> 2) & 1)));
    xv[v][0] = xverts[vi * 3 + 0];
    xv[v][1] = xverts[vi * 3 + 1];
    xv[v][2] = xverts[vi * 3 + 2];
  }
  double G9[9], d;
  hex_point_geometry(xv, pts[i], pts[j], pts[k], wts[i] * wts[j] * wts[k], use_fabs, do_clamp,
                     G6blk ? G9 : nullptr, &d);
  if (cell_coeff) scale_point_geometry(cell_coeff[c], G6blk ? G9 : nullptr, &d);
  if (mdiag) {
    const size_t NX = (size_t)P * nx + 1, NY = (size_t)P * ny + 1;
    const size_t g = (size_t)(P * cx + i) + NX * ((size_t)(P * cy + j) + NY * (size_t)(P * cz + k));
    unsafeAtomicAdd(&mdiag[g], d);
  }
  if (G6blk) {
    const int nbx = (nx + bx - 1) / bx, nby = (ny + by - 1) / by;
    const int Bx = cx / bx, By = cy / by, Bz = cz / bz;
    const size_t blk = (size_t)Bx + (size_t)nbx * (By + (size_t)nby * Bz);
    const int cl = (cx % bx) + bx * ((cy % by) + by * (cz % bz));
    const int CB = bx * by * bz;
    store_g6(G6blk, n, CB * n * n, blk, k, cl * n * n + j * n + i, G9);
  }
}

// --------------------------------------------------------------------------
// launchers
// --------------------------------------------------------------------------
int launch_geometry_hex(int P, int ncells, const double* d_xverts, const int32_t* d_geom_dofmap,
                        const double* d_pts, const double* d_wts, int use_fabs, int clamp, double* d_G9,
                        double* d_G6blk, double* d_detJ, const double* d_cell_coeff, hipStream_t s)
{
  const int n = P + 1;
  const size_t N = (size_t)ncells * n * n * n;
  if (N == 0) return WF_OK;
  hipLaunchKernelGGL(k_geometry_hex, dim3(grid_for(N, 256)), dim3(256), 0, s, n, cells_per_batch(P), ncells,
                     d_xverts, d_geom_dofmap, d_pts, d_wts, use_fabs, clamp, d_G9, d_G6blk, d_detJ, d_cell_coeff);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_geometry_hex_slots(int P, int CB, int ncells, const double* d_xverts, const int32_t* d_geom_dofmap,
                              const int32_t* d_slot_of, const uint8_t* d_sign, const double* d_pts, const double* d_wts,
                              int use_fabs, int clamp, double* d_G6blk, const double* d_cell_coeff, hipStream_t s)
{
  const int n = P + 1;
  const size_t N = (size_t)ncells * n * n * n;
  if (N == 0) return WF_OK;
  hipLaunchKernelGGL(k_geometry_hex_slots, dim3(grid_for(N, 256)), dim3(256), 0, s, n, CB, ncells,
                     d_xverts, d_geom_dofmap, d_slot_of, reinterpret_cast<const int8_t*>(d_sign), d_pts, d_wts, use_fabs,
                     clamp, d_G6blk, d_cell_coeff);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_pack_G6(int P, int CB, int ncells, const double* d_G9, double* d_G6blk, hipStream_t s)
{
  const int n = P + 1;
  const size_t N = (size_t)ncells * n * n * n;
  if (N == 0) return WF_OK;
  hipLaunchKernelGGL(k_pack_G6, dim3(grid_for(N, 256)), dim3(256), 0, s, n, CB, ncells, d_G9,
                     d_G6blk);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

int launch_geometry_box(int P, int nx, int ny, int nz, int bx, int by, int bz, const double* d_xverts,
                        const double* d_pts, const double* d_wts, int use_fabs, int clamp, double* d_G6blk,
                        double* d_mdiag, const double* d_cell_coeff, hipStream_t s)
{
  const int n = P + 1;
  const size_t N = (size_t)nx * ny * nz * n * n * n;
  if (N == 0) return WF_OK;
  hipLaunchKernelGGL(k_geometry_box, dim3(grid_for(N, 256)), dim3(256), 0, s, n, nx, ny, nz, bx, by, bz,
                     d_xverts, d_pts, d_wts, use_fabs, clamp, d_G6blk, d_mdiag, d_cell_coeff);
  WF_LAUNCH_CHECK();
  return WF_OK;
}

}  // namespace wf
