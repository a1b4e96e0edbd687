/*
 * wavehip.h -- C ABI of libwavehip, the MI355X (gfx950) matrix-free operator
 * engine for the explicit-RK wave loop of Excalibur-SLE/wave-fenics.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types,
 * no exceptions.  Every entry point returns 0 on success or a negative
 * wf_status; wf_last_error() returns the message of the last failure on the
 * calling thread.  Each declaration cites the reference interface it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - fp64 data, int32 indices.
 *   - "h_" parameters are host pointers read during the call (setup);
 *     "d_" parameters are device pointers (hipMalloc / torch tensors).
 *   - apply is y += A x (the reference accumulates, operators.hpp:196-198,
 *     scatter.cu:43; the caller zeroes y, LinearGLL.hpp:173).
 *   - stream is a hipStream_t passed as void* (NULL = default stream); all
 *     device work is stream-ordered and asynchronous, nothing synchronises
 *     except wf_sync, the two calls that hand results to the host (wf_comm_barrier,
 *     wf_cg: both synchronise `stream`) and the setup calls that read host memory
 *     (the create calls allocate and copy synchronously: keep them out of a step loop).
 *   - element-local tensor ordering l = i + n*(j + n*k), n = P+1, i along x (x FASTEST).
 *     This is the order of every per-dof / per-point array handed over: the tensor side
 *     of h_perm, h_dofmap when h_perm is NULL, the point index q of h_G [c][q][3][3] and
 *     h_detJ [c][q], and the vertex index v = a + 2b + 4c of h_geom_dofmap.  A caller whose
 *     tensor order is x SLOWEST (Basix' get_tensor_product_representation, whose perm the
 *     reference uses as is, common/permute.hpp:12-17, spectral_mass.hpp:36-38) sets
 *     WF_FLAG_TENSOR_X_SLOWEST; pairing an x-slowest index with this engine's x-fastest
 *     geometry silently mixes G_xx with G_zz on any non-cubic cell.
 */
#ifndef WAVEHIP_H
#define WAVEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  WF_OK = 0,
  WF_ERR_INVALID = -1,     /* bad argument                                      */
  WF_ERR_UNSUPPORTED = -2, /* e.g. degree outside 1..7 (mass.hpp:91-92 throws)  */
  WF_ERR_HIP = -3,         /* a HIP runtime call failed (array.hpp:15-17 throws) */
  WF_ERR_NODEVICE = -4,    /* fewer devices than requested (utils.hpp:30-34)     */
  WF_ERR_COMM = -5         /* RCCL missing or a communication call failed
                              (the reference asserts on MPI status, VectorUpdater.hpp:120) */
} wf_status;

typedef struct wf_op wf_op;

const char* wf_last_error(void);
const char* wf_version(void);

/* ---- device runtime shims: common/cuda/utils.hpp:22-56, array.hpp:8-51 ---- */
int wf_device_count(int* count);
int wf_set_device(int device);                       /* utils::set_device      */
int wf_device_info(int device, char* name, size_t name_len, size_t* total_mem,
                   int* num_cu);                     /* utils::output_device_info */
int wf_malloc(void** d_ptr, size_t bytes);           /* cuda::array ctor       */
int wf_free(void* d_ptr);                            /* cuda::array dtor       */
int wf_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes); /* array::set */
int wf_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes); /* copy_to_host */
int wf_memset(void* d_dst, int value, size_t bytes, void* stream);
int wf_sync(void* stream);                           /* cudaDeviceSynchronize  */

/* ---- a1/a13: tabulation (host) ------------------------------------------
 * common/operators.hpp:13-32 tabulate_basis_and_permutation,
 * common/precompute.hpp:179-189 tabulate_1d.
 * 1-D GLL rule with P+1 points on [0,1] and the collocation derivative matrix
 * D[q*n + a] = l_a'(xi_q), clamped to -1/0/1 like the reference's dense table.
 * Any output pointer may be NULL. */
int wf_tabulate_gll(int P, double* h_points, double* h_weights, double* h_D);

/* 1-D quadrature rules as basix::quadrature::make_quadrature(type, interval, degree)
 * selects them (common/precompute.hpp:183-184, demo/gpu_operator/main.cpp:96-99,
 * common/operators.hpp:19): Gauss-Jacobi (alpha = beta = 0, i.e. Gauss-Legendre) with
 * (degree+2)/2 points, GLL with (degree+4)/2 points; on [0,1], ascending.
 * *npts is always set; h_points / h_weights (capacity WF_MAX_QUAD_POINTS) may be NULL. */
typedef enum { WF_QUAD_GLL = 0, WF_QUAD_GAUSS_JACOBI = 1 } wf_quadrature_type;
typedef enum { WF_VARIANT_GLL_WARPED = 0, WF_VARIANT_EQUISPACED = 1 } wf_lagrange_variant;
#define WF_MAX_QUAD_POINTS 16
int wf_quadrature_1d(int type, int degree, int* npts, double* h_points, double* h_weights);

/* common/precompute.hpp:179-189 tabulate_1d: the degree-P Lagrange basis of the given
 * variant on the interval at npts points; h_table[q*(P+1) + a] = l_a(x_q) (derivative 0)
 * or l_a'(x_q) (derivative 1).  Not clamped (neither is the reference's). */
int wf_tabulate_1d(int P, int variant, int npts, const double* h_points, int derivative, double* h_table);

/* Dense reference-layout table[4][nq][nd] (0 = values, 1..3 = d/dx,d/dy,d/dz),
 * nq = nd = (P+1)^3, tensor ordering, clamped (operators.hpp:23-29). */
int wf_tabulate_dense(int P, double* h_table);

/* common/permute.hpp:10-27 reorder_dofmap: out[c*nd + k] = in[c*nd + perm[k]]. */
int wf_reorder_dofmap(int ncells, int nd, const int32_t* h_perm,
                      const int32_t* h_in, int32_t* h_out);

/* Setup-time renumbering option: a dof numbering that follows the lattice columns the marching kernels walk
 * (work items in z-segment / column order, inside an item plane by plane, row by row), for spaces whose own
 * numbering scatters a cell's dofs over memory.  The reference takes DOLFINx's numbering as it comes
 * (fem::create_functionspace, demo/cpu_planar3d/main.cpp:47-52, reordered by DOLFINx's graph reordering); a
 * caller applies h_new_of_old to its dofmap and vectors before creating operators.  Host only.
 * h_dofmap: tensor-ordered (x fastest) [ncells][(degree+1)^3]; h_new_of_old[ndofs]. */
int wf_lattice_numbering(int degree, int64_t ncells, int32_t ndofs, const int32_t* h_dofmap, int32_t* h_new_of_old);

/* ---- a2/a13: geometry (device kernel, host in/out) -----------------------
 * common/precomputation.hpp:18-110 precompute_geometric_data (use_fabs = 1,
 * clamp = 1) and common/precompute.hpp:49-176 (use_fabs = 0, clamp = 0).
 * h_xverts [nverts][3], h_geom_dofmap [ncells][8] (vertex v = a + 2b + 4c).
 * Outputs in the reference layout: h_G [ncells][nq][3][3] (may be NULL),
 * h_detJ [ncells][nq] (may be NULL); quadrature = (P+1)^3 GLL points. */
int wf_geometry_hex(int P, int ncells, int nverts, const double* h_xverts,
                    const int32_t* h_geom_dofmap, int use_fabs, int clamp,
                    double* h_G, double* h_detJ);

/* The generic helpers of common/precompute.hpp:49-176 (compute_jacobian, _determinant,
 * _inverse, compute_geometrical_factor) at an arbitrary tensor-product rule
 * nq1 x nq1 x nq1 (point q = i + nq1*(j + nq1*k), weight w_i w_j w_k):
 * h_detJ [ncells][nq1^3] = det J * w (|det J| * w with use_fabs), h_G [ncells][nq1^3][3][3]
 * = K K^T detJ w.  Either output may be NULL. */
int wf_geometry_hex_rule(int ncells, int nverts, const double* h_xverts, const int32_t* h_geom_dofmap, int nq1,
                         const double* h_points1, const double* h_weights1, int use_fabs, int clamp, double* h_G,
                         double* h_detJ);
/* Per-cell geometry of affine hexahedra and the test that decides whether a stiffness operator may store it (host
 * only; the rule of wf_op_create_box and of wf_op_create with WF_GEOMETRY_PER_CELL).  A cell qualifies when its edge
 * vectors along each reference axis are bitwise equal, det J is non-zero and finite, and -- with clamp -- the reference's
 * -1/0/1 clamp changes neither a cmap derivative at the degree-P GLL points nor a component of any G_c w_i w_j w_k.
 * h_Gc [ncells][6] = G00 G01 G02 G11 G12 G22 of G_c = J^-1 J^-T |det J| (det J signed without use_fabs; weights left
 * out), may be NULL; it is complete when every cell qualifies.  *first_bad = -1 then, else the first cell that does not;
 * *reason says why (0 ok, 1 not affine, 2 det J zero / not finite, 3 the clamp would take effect).  Returns WF_OK
 * either way. */
int wf_geometry_hex_cell(int P, int64_t ncells, int64_t nverts, const double* h_xverts, const int32_t* h_geom_dofmap,
                         int use_fabs, int clamp, double* h_Gc, int64_t* first_bad, int* reason);

/* ---- operators -----------------------------------------------------------*/
typedef enum {
  WF_OP_STIFFNESS = 0,   /* StiffnessOperator      common/operators.hpp:137-201 */
  WF_OP_MASS_LUMPED = 1, /* MassOperatorCPU / SpectralMassOperator
                            common/operators.hpp:44-109, cuda/spectral_mass.hpp:24-100 */
  WF_OP_MASS_DENSE = 2   /* MassOperator (Phi^T D Phi) common/cuda/mass.hpp:18-107    */
} wf_op_kind;

typedef enum {
  WF_FLAG_NONE = 0,
  WF_FLAG_NO_FABS = 1,     /* detJ keeps its sign (spectral_mass.hpp:58-64)    */
  WF_FLAG_NO_CLAMP = 2,    /* skip the -1/0/1 clamp of G                        */
  WF_FLAG_TENSOR_X_SLOWEST = 8, /* the caller's tensor index -- the domain of h_perm (or of
                              h_dofmap when h_perm is NULL) and the point index of h_G /
                              h_detJ -- is l' = (i n + j) n + k with i along x, the order of
                              Basix' tensor-product factorisation, instead of the engine's
                              l = i + n (j + n k).  The 3x3 axes of G are reference axes
                              0, 1, 2 = x, y, z in both conventions.                   */
  WF_FLAG_MASS_ELEMENTWISE = 4, /* lumped mass with a dofmap: apply as the reference's
                              gather * detJ -> scatter-add per cell
                              (spectral_mass.hpp:84-89) instead of the pre-assembled
                              diagonal y += m .* x (m = M 1 built once at create)  */
  WF_FLAG_ORDERED = 16     /* order-fixed accumulation: y is a pure function of the inputs (bitwise
                              reproducible on any mesh, no atomics).  See "Order-fixed accumulation"
                              below.                                                            */
} wf_flags;

/* Order-fixed accumulation (WF_FLAG_ORDERED).  Two passes: pass 1 writes every cell's element-local
 * result with plain stores, pass 2 gives every y entry to one thread, which sums that entry's
 * contributions in a fixed order and reads and writes y[d] once.
 * The order contract: the contributions of dof d are the entries of the caller's h_dofmap equal to d, in
 * the order in which they appear when h_dofmap is read front to back (ascending cell index in the caller's
 * numbering, then position within the cell's row); y[d] = y[d] + (((v_0 + v_1) + v_2) + ...); a dof no
 * cell lists keeps its y.  Internal cell sorting and batch composition do not enter, nor does the dof
 * numbering: relabelling the dofs relabels y bitwise.
 *   wf_op_create         stiffness (P1 to P7, per-point geometry), dense mass (any tensor rule), lumped mass with
 *                        WF_FLAG_MASS_ELEMENTWISE: kernel WF_KERNEL_CELLS_ORDERED, update WF_UPDATE_ORDERED.  Lumped mass
 *                        without it: the kernel stays WF_KERNEL_DIAGONAL, the diagonal m = M 1 is assembled in that order
 *                        (two creations give a bitwise equal m).
 *   wf_op_create_box*    builds the box's lexicographic dofmap and vertex map on the host and is then that dofmap operator
 *                        (wf_op_info_t.structured stays 1).
 *   wf_op_create_dense_simplex, wf_op_create_dense_simplex_mass   WF_ERR_UNSUPPORTED.
 * Any non-default wf_tuning field other than keep_cell_order is WF_ERR_INVALID together with the flag (there is no kernel
 * to choose); wf_op_set_ghost_faces / _dofs are WF_ERR_UNSUPPORTED as for the batch kernels.  The operator owns the
 * scratch v[ncells * nd] (counted in device_bytes): ONE APPLY PER OPERATOR MAY BE IN FLIGHT AT A TIME -- applies of one
 * handle on different streams must be ordered by the caller.  alg_bytes is the default form's formula plus
 * 20 ncells nd + 4 (ndofs + 1).  wf_dot / wf_cg keep their own cross-workgroup atomics. */

/* Which kernel an operator runs (wf_op_info_t.kernel) ... */
typedef enum {
  WF_KERNEL_NONE = 0,
  WF_KERNEL_MARCH_BOX = 1,      /* k_stiffness_march: box mesh, implicit dofmap (stiffness_march.hip)       */
  WF_KERNEL_MARCH_IDX = 2,      /* k_march_idx: lattice columns of any dofmap (stiffness_march_idx.hip)     */
  WF_KERNEL_BATCH_UNIQUE = 3,   /* k_stiffness_generic_u / k_mass_lumped_u / k_mass_dense_col: batches of
                                   cells with a unique-dof tile -- what a mesh that does not tile gets     */
  WF_KERNEL_BOX_BLOCK = 4,      /* k_stiffness_box: one block of cells per workgroup, single pass           */
  WF_KERNEL_DIAGONAL = 5,       /* pre-assembled lumped mass, y += m .* x                                   */
  WF_KERNEL_MASS_DENSE_ANY = 6, /* k_mass_dense: any tensor rule (nq1 != P+1 allowed)                       */
  WF_KERNEL_DENSE_SIMPLEX = 7,  /* k_stiffness_dense: MFMA fp64, affine simplices                           */
  WF_KERNEL_ELEMENTWISE = 8,    /* k_mass_lumped: one thread per element-local dof                          */
  WF_KERNEL_CELLS_ORDERED = 9,  /* WF_FLAG_ORDERED: cell batches store element-local results, one thread per y
                                   entry sums them in a fixed order (ordered.hip)                           */
  WF_KERNEL_DENSE_SIMPLEX_MASS = 10 /* k_mass_dense_simplex: MFMA fp64, affine simplices, y += s_c A x       */
} wf_kernel_id;

/* ... and the explicit, thread-safe way to select one (tests, tuning runs).  Every field 0 =
 * the library's own choice; a NULL wf_tuning* means all defaults.  The library reads no
 * environment variable when it creates or applies an operator. */
typedef enum {
  WF_KERNEL_AUTO = 0,
  WF_KERNEL_FORCE_BATCH = 1,      /* skip the lattice-column plan: the batch kernels                        */
  WF_KERNEL_FORCE_BOX_BLOCK = 2,  /* box stiffness: the single-pass block kernel instead of marching        */
  WF_KERNEL_FORCE_MASS_ANY = 3,   /* dense mass: the any-rule kernel even for square tables                 */
  WF_KERNEL_FORCE_ELEMENTWISE = 4,/* batch kernels without the unique-dof tile (element-wise atomics)       */
  WF_KERNEL_FORCE_MARCH = 5,      /* adopt the lattice-column plan whatever its fill (default: plans whose
                                     columns are mostly empty keep the batch kernel)                        */
  WF_KERNEL_FORCE_MASS_MARCH = 6  /* dense mass with a rectangular table (nq1 != P+1): the marching kernel
                                     k_mass_march instead of k_mass_dense -- see below                      */
} wf_kernel_hint;
/* WF_KERNEL_FORCE_MASS_MARCH.  A dense mass whose 1-D table is rectangular runs k_mass_dense (WF_KERNEL_MASS_DENSE_ANY)
 * under every other hint; the marching kernel takes it on request only.  WF_OP_MASS_DENSE with nq1 != P+1 and a
 * compiled pair (P, nq1): the lattice-column plan is built as for WF_KERNEL_FORCE_MARCH -- adopted whatever its fill,
 * wf_tuning.lz, bx / by (a compiled cross-section of the pair, else its default) and orient honoured; cell
 * orientations are normalised only when the table reads the same backwards, phi1[nq1-1-q][P-a] == phi1[q][a].
 * wf_op_info_t then reports kernel = WF_KERNEL_MARCH_IDX, the plan_* fields, num_quads = nq1^3, and flops and
 * alg_bytes by the formulas of every dense mass.  Compiled pairs (P, nq1): Gauss rules of degree 2P+2, (1,3) (2,4)
 * (3,5) (4,6) (5,7) (6,8); the GLL rule of degree P+1 where it is not square, (4,4) (5,5) (6,5) (7,6).  Cross-sections
 * other than the default: 2x2 at (4,6) and (4,4), 2x1 at (6,8) and (6,5).  A cell must fit one wavefront
 * (max(P+1, nq1) <= 8).  With nq1 == P+1 the hint is WF_KERNEL_FORCE_MARCH.
 * Errors: a stiffness or lumped-mass operator with the hint is WF_ERR_INVALID; a pair that is not compiled, or a mesh
 * that does not tile into lattice columns, is WF_ERR_UNSUPPORTED (wf_last_error names (P, nq1)); together with
 * WF_FLAG_ORDERED it is WF_ERR_INVALID like every other hint.  wf_op_set_ghost_dofs stays WF_ERR_UNSUPPORTED for
 * mass operators. */
typedef struct {
  int kernel;        /* wf_kernel_hint                                                              */
  int variant;       /* box marching kernel: compiled column cross-section + 1 (0 = default); with
                        the owner update it indexes the owner form's cross-sections (3 per degree)  */
  int lz;            /* layers per z segment of the marching kernels (0 = chosen from the mesh)     */
  int lz0;           /* length of the first z segment under a z ghost plane (0 = 3)                 */
  int bx, by, bz;    /* cells per block of the single-pass box kernel (0 = default)                 */
  int keep_cell_order; /* batch kernels: do not sort the cells by their smallest dof                */
  int orient;        /* lattice plan: 0 = normalise cell orientations (default), 1 = require the
                        cells to agree as given                                                     */
  int geometry;      /* box stiffness, P <= 4 marching kernel (P5 to P7: with update = OWNER only):
                        wf_geometry_mode.  wf_op_create, stiffness at P <= 4: PER_CELL on request
                        only (AUTO = PER_POINT there); no effect on the mass operators              */
  int metric;        /* stiffness with per-cell geometry (box or wf_op_create): wf_metric_mode      */
  int update;        /* box stiffness, separable (axes) form: wf_update_mode; OWNER on request at
                        P1 to P7.  wf_op_create with PER_CELL: OWNER is WF_ERR_UNSUPPORTED          */
} wf_tuning;
/* How a stiffness operator stores its geometry (wf_tuning.geometry, wf_op_info_t.geometry).  A box
 * whose cells are all affine (edge vectors along each reference axis bitwise equal, det J != 0, no
 * -1/0/1 clamp taking effect) needs one G_c = J^-1 J^-T |det J| per cell instead of one G per point.
 * At P5 to P7 the only per-cell kernel is the owner form (wf_tuning.update = WF_UPDATE_OWNER); without that
 * request the k-split kernel runs on per-point geometry and PER_CELL is WF_ERR_UNSUPPORTED.
 * wf_op_create (any dofmap, the lattice-column plan, stiffness at P1 to P4) stores per-cell geometry on request only:
 * AUTO and PER_POINT keep G per point.  PER_CELL there derives G_c from the mesh (wf_geometry_hex_cell) and adopts the
 * plan whatever its fill; it is WF_ERR_INVALID for a cell that does not qualify (wf_last_error names it), without a mesh,
 * or with a batch kernel hint, and WF_ERR_UNSUPPORTED at P >= 5, with h_G, with WF_UPDATE_OWNER, or on a mesh that does
 * not tile into lattice columns. */
typedef enum {
  WF_GEOMETRY_AUTO = 0,       /* tuning: box: per cell where the mesh allows it; wf_op_create: per point;
                                 info: no stiffness geometry                                            */
  WF_GEOMETRY_PER_POINT = 1,  /* G at every quadrature point (48 B each)                                */
  WF_GEOMETRY_PER_CELL = 2    /* one G_c per affine cell (48 B); tuning: WF_ERR_INVALID if not affine   */
} wf_geometry_mode;
/* Which form of the per-cell box kernel runs (wf_tuning.metric, wf_op_info_t.metric).  When every G_c is
 * diagonal (a rectilinear box: off-diagonals exactly 0) the cell operator separates into one 1-D operator
 * A = D^T diag(w) D per axis, which takes about half the LDS reads and FMAs of the full tensor.
 * The same holds for wf_op_create with WF_GEOMETRY_PER_CELL; diagonal is decided on every cell's G_c (a cell's own frame
 * and the plan's frame differ by a signed permutation of the axes). */
typedef enum {
  WF_METRIC_AUTO = 0,         /* tuning: axes where every G_c is diagonal, else full                   */
  WF_METRIC_NONE = 0,         /* info: no per-cell geometry                                            */
  WF_METRIC_FULL = 1,         /* the full-tensor per-cell form (tuning: also on rectilinear boxes)     */
  WF_METRIC_AXES = 2          /* the separable form; tuning: WF_ERR_INVALID if a G_c is not diagonal,
                                 WF_ERR_UNSUPPORTED without per-cell geometry                         */
} wf_metric_mode;
/* How the separable box kernel adds its result into y (wf_tuning.update, wf_op_info_t.update).  The atomic
 * form adds each column's tile with fp64 atomics; the owner form gives every y entry to one thread, which
 * gathers it from the cells around the node and reads and writes it once (no atomics, a fixed summation
 * order: bitwise reproducible).  wf_tuning.variant then indexes the owner form's own cross-sections.
 * The owner form is compiled for P1 to P7; the atomic separable form for P1 to P4. */
typedef enum {
  WF_UPDATE_AUTO = 0,         /* tuning: owner at P4, atomic at P1 to P3; P5 to P7: the k-split kernel
                                 on per-point geometry (the owner form there is on request only)       */
  WF_UPDATE_NONE = 0,         /* info: not the separable box kernel                                     */
  WF_UPDATE_ATOMIC = 1,       /* row atomics (also the only form of the full and per-point kernels, and of
                                 the per-cell forms of wf_op_create)                                    */
  WF_UPDATE_OWNER = 2,        /* owner computes (P1 to P7); tuning: WF_ERR_UNSUPPORTED unless the axes
                                 form runs (a rectilinear box)                                          */
  WF_UPDATE_ORDERED = 3       /* info only (WF_FLAG_ORDERED operators); wf_tuning.update = 3 stays an error */
} wf_update_mode;

typedef struct {
  int kind;                    /* wf_op_kind                                    */
  int degree;                  /* P in 1..7, hexahedron, nd = (P+1)^3           */
  int ncells;                  /* local cells (operators.hpp:153)                */
  int ndofs;                   /* length of x and y: owned + ghost dofs          */
  const int32_t* h_dofmap;     /* [ncells][nd], element ordering                 */
  const int32_t* h_perm;       /* tensor -> element ordering (the reference's
                                  `perm`, operators.hpp:24); NULL = identity      */
  /* geometry: either precomputed arrays in the reference layout ...            */
  const double* h_G;           /* [ncells][nq][3][3] (stiffness) or NULL         */
  const double* h_detJ;        /* [ncells][nq] (mass) or NULL                    */
  /* ... or the mesh, in which case the geometry is computed on the device      */
  int nverts;
  const double* h_xverts;      /* [nverts][3]                                    */
  const int32_t* h_geom_dofmap;/* [ncells][8]                                    */
  double c0;                   /* speed of sound; stiffness carries -c0^2
                                  (operators.hpp:114-115; reference fixes 1500)   */
  int flags;                   /* wf_flags                                       */
  /* WF_OP_MASS_DENSE only: 1-D interpolation matrix phi1[nq1][P+1] (row-major)
   * of a tensor-product rule; h_detJ is then [ncells][nq1^3].                   */
  int nq1;
  const double* h_phi1;
  /* WF_OP_MASS_DENSE with the mesh instead of h_detJ: the 1-D rule (points, weights
   * [nq1]) at which det J * w is computed on the device (mass.hpp:35-39).        */
  const double* h_qpts1;
  const double* h_qwts1;
  const wf_tuning* tuning;     /* NULL = defaults                                */
  const double* h_cell_coeff;  /* [ncells] cell coefficient a_c, rows of h_dofmap; NULL = none
                                  (see "Cell coefficients" below)                 */
} wf_op_desc;

/* Op(V, degree[, params]) constructors: operators.hpp:53,149; mass.hpp:20;
 * spectral_mass.hpp:26.  Copies every host array; owns all device state. */
int wf_op_create(const wf_op_desc* desc, wf_op** out);

/* Structured box mesh (mesh::create_box, demo/gpu_operator/main.cpp:60-63) with
 * this engine's lexicographic numbering: vertex (a,b,c) -> a + (nx+1)(b + (ny+1)c),
 * dof (I,J,K) -> I + NX*(J + NY*K), NX = P*nx+1 ...  The dofmap is implicit
 * (never read from memory) and the geometry is computed on the device from
 * h_xverts [(nx+1)(ny+1)(nz+1)][3]. */
int wf_op_create_box(int kind, int degree, int nx, int ny, int nz,
                     const double* h_xverts, double c0, int flags, wf_op** out);
int wf_op_create_box_tuned(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0, int flags,
                           const wf_tuning* tuning, wf_op** out);
/* The box operator with a cell coefficient h_cell_coeff[nx ny nz], cell (cx, cy, cz) -> cx + nx (cy + ny cz); NULL gives
 * the operator of the two entry points above, which are calls of this one. */
int wf_op_create_box_coeff(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0,
                           const double* h_cell_coeff, int flags, const wf_tuning* tuning, wf_op** out);

/* Cell coefficients (heterogeneous media).  An operator created with h_cell_coeff applies
 *   y += sum_c a_c P_c^T A_c P_c x,
 * A_c the cell matrix of the operator without a coefficient -- for the stiffness operator with its -c0^2 factor and the
 * reference's -1/0/1 clamp, both applied before a_c.  a_c is one double per cell in the caller's cell order: the rows of
 * h_dofmap / h_geom_dofmap, on a box cx + nx (cy + ny cz).  The array is copied at creation; a medium cannot be changed
 * afterwards, and a coefficient that varies inside a cell is out of scope.
 *   - Every a_c must be finite; zero and negative values are allowed.  A NaN or infinite entry is WF_ERR_INVALID and
 *     wf_last_error names the first such cell.  The check precedes the first device call.
 *   - Hexahedral operators and the tetrahedral mass FOLD the coefficient into the geometry they store: every stored entry
 *     (G per point, G_c per cell, det J w, s_c, the lumped diagonal's det J w before it is accumulated, the caller's h_G /
 *     h_detJ) is the entry of the operator without a coefficient multiplied once by a_c and rounded once.  The apply reads
 *     the same arrays with the same kernels: a heterogeneous medium costs what a homogeneous one costs.
 *   - The tetrahedral stiffness forms clamp(w_q C_c) on the fly, so a coefficient folded into C_c would move the clamp
 *     windows: its kernel has a variant that loads a_c next to C_c and scales by -c0^2 a_c after the clamp.  Its
 *     alg_bytes is that of the operator without a coefficient plus 8 ncells.
 *   - The coefficient does not enter kernel selection: kernel, geometry, metric, update, the plan fields and (but for the
 *     tetrahedral stiffness) alg_bytes are those of the operator without it; the affine-cell test, the axes-form test and
 *     the run-table tuning see the geometry without the coefficient.
 *   - WF_FLAG_ORDERED: y stays a pure function of the inputs, the coefficient being one of them.
 * With NULL no scaling step runs and no array is touched: the operator is bit for bit the one without the field. */

/* Dense (non-tensor-product) stiffness operator on affine simplex cells: the
 * reference's skernel (common/operators.hpp:113-133) fed with arbitrary dense
 * tables, as its cell loop (operators.hpp:183-200) would be for a tetrahedral
 * space.  h_dphi is the table the reference keeps as `_dphi` (operators.hpp:178):
 * [3][nq][nd], already clamped by the caller like operators.hpp:27-29;
 * h_weights [nq]; cells are affine tetrahedra given by h_geom_dofmap [ncells][4].
 * G = (J^-1 |det J| w_q) J^-T with the -1/0/1 clamp is formed on the fly
 * (precomputation.hpp:95-107).  Compiled shapes: Lagrange P1..P4; any other (nd, nq) with
 * the same tile counts ceil(nq/16), ceil(nd/4), ceil(nd/16) runs too, the rest is
 * WF_ERR_UNSUPPORTED at creation.
 * A degenerate cell (det J zero or not finite) is WF_ERR_INVALID at creation. */
typedef struct {
  int nd, nq;                   /* dofs and quadrature points per cell            */
  int ncells, ndofs;
  const int32_t* h_dofmap;      /* [ncells][nd]                                   */
  const double* h_dphi;         /* [3][nq][nd]                                    */
  const double* h_weights;      /* [nq]                                           */
  int nverts;
  const double* h_xverts;       /* [nverts][3]                                    */
  const int32_t* h_geom_dofmap; /* [ncells][4]                                    */
  double c0;
  int flags;                    /* WF_FLAG_NO_CLAMP; WF_FLAG_ORDERED: WF_ERR_UNSUPPORTED */
  const double* h_cell_coeff;   /* [ncells] cell coefficient a_c or NULL ("Cell coefficients"): applied inside the
                                   kernel, after -c0^2 and the clamp; alg_bytes grows by 8 ncells            */
} wf_dense_desc;
int wf_op_create_dense_simplex(const wf_dense_desc* desc, wf_op** out);

/* Dense (non-tensor-product) mass operator on affine simplex cells: the reference's MassOperator
 * (common/cuda/mass.hpp:18-107, y_e = Phi^T (det J w .* (Phi x_e))) fed with an arbitrary dense table, as it would
 * be for a tetrahedral space.  h_phi is the table of basis VALUES at the quadrature points, [nq][nd], taken as it
 * is (mass.hpp tabulates values: there is no -1/0/1 clamp); h_weights [nq]; cells are affine tetrahedra given by
 * h_geom_dofmap [ncells][4].  det J is constant on an affine cell, so the operator is applied as
 *   y[dofmap[c][a]] += s_c sum_b A[a][b] x[dofmap[c][b]],   A = Phi^T diag(w) Phi,
 * with A formed once on the host (long double, rounded once) and s_c = |det J_c|, or det J_c with its sign under
 * WF_FLAG_NO_FABS (mass.hpp:35-39).  The cost of an apply does not depend on nq: any nq >= 1 is accepted.
 * Compiled shapes: the tile counts ceil(nd/4), ceil(nd/16) of Lagrange P1..P4 (nd = 4, 10, 20, 35), which serve
 * nd = 1..4, 9..12, 17..20 and 33..36; every other nd is WF_ERR_UNSUPPORTED at creation.  A degenerate cell (det J
 * zero or not finite) is WF_ERR_INVALID at creation, wf_last_error names the cell.  All argument checks precede the
 * first device call.  wf_op_info_t: kind WF_OP_MASS_DENSE, degree 0, kernel WF_KERNEL_DENSE_SIMPLEX_MASS, flops by the
 * reference's model 4 ncells nq nd (mass.hpp:71), alg_bytes = ncells (8 + 4 nd) + 16 ndofs.  wf_op_apply_part (any
 * part but WF_PART_ALL) and wf_op_set_ghost_* are WF_ERR_UNSUPPORTED: a batch kernel.  wf_cg takes the handle as it is
 * (M a = b, the problem of demo/gpu_cg on a tetrahedral space). */
typedef struct {
  int nd, nq;                   /* dofs and quadrature points per cell            */
  int ncells, ndofs;
  const int32_t* h_dofmap;      /* [ncells][nd]                                   */
  const double* h_phi;          /* [nq][nd], not clamped                          */
  const double* h_weights;      /* [nq]                                           */
  int nverts;
  const double* h_xverts;       /* [nverts][3]                                    */
  const int32_t* h_geom_dofmap; /* [ncells][4]                                    */
  int flags;                    /* WF_FLAG_NO_FABS; WF_FLAG_ORDERED: WF_ERR_UNSUPPORTED; any other bit: WF_ERR_INVALID */
  const double* h_cell_coeff;   /* [ncells] cell coefficient a_c or NULL ("Cell coefficients"): folded into s_c */
} wf_dense_mass_desc;
int wf_op_create_dense_simplex_mass(const wf_dense_mass_desc* desc, wf_op** out);

/* op(x, y) / op.apply(x, y): y += A x.  operators.hpp:183, mass.hpp:76,
 * spectral_mass.hpp:84. */
int wf_op_apply(wf_op* op, const double* d_x, double* d_y, void* stream);

/* Interior / interface split of a stiffness operator on a domain-decomposed mesh: lets the
 * caller overlap the ghost updates (VectorUpdater::update_fwd_begin/_end and update_rev,
 * demo/gpu_scatter_mpi/VectorUpdater.hpp:106-143,157-199) with the work that touches no ghost
 * dof.  The operator's work items (columns of cells, stiffness_march*.hip) are sorted into
 * INTERFACE (the item's dof tile contains a ghost position) and INTERIOR;
 * apply(INTERIOR) + apply(INTERFACE) == apply.
 *   wf_op_set_ghost_dofs : any marching operator (box or arbitrary dofmap), ghosts given as
 *                          positions in the local array -- the same list the updater gets
 *                          (wf_updater_desc.ghost_positions, any order, duplicates allowed);
 *                          on a box operator the first z segment is short (wf_tuning.lz0) when every
 *                          position of the lattice plane K = 0 is a ghost, as with ghost_z0 below, so
 *                          that the same planes give the same work items through either call;
 *   wf_op_set_ghost_faces: box operators, ghosts = the lower lattice plane of the marked axes
 *                          (the Cartesian partition of SURVEY 8e).
 * WF_ERR_UNSUPPORTED for operators that run a batch kernel (no work items to sort). */
typedef enum {
  WF_PART_ALL = 0,
  WF_PART_INTERIOR = 1,    /* every work item that touches no ghost dof                   */
  WF_PART_INTERFACE = 2,
  WF_PART_INTERIOR_A = 3,  /* INTERIOR split in two halves: A hides the forward halo,    */
  WF_PART_INTERIOR_B = 4   /* B the reverse (add) halo; A + B == INTERIOR                */
} wf_part;
int wf_op_set_ghost_faces(wf_op* op, int ghost_x0, int ghost_y0, int ghost_z0);
int wf_op_set_ghost_dofs(wf_op* op, const int32_t* h_ghost_positions, int32_t nghosts);
int wf_op_apply_part(wf_op* op, const double* d_x, double* d_y, int part, void* stream);

typedef struct {
  int kind, degree, num_cells, num_dofs_cell, num_quads, ndofs, structured;
  double flops;          /* reference model 4*ncells*nq*nd (mass.hpp:71)        */
  double alg_bytes;      /* algorithmic HBM bytes per apply          */
  size_t device_bytes;   /* device memory owned by the operator                  */
  int items_interior, items_interface; /* work items per part (wf_op_set_ghost_*)     */
  int kernel;            /* wf_kernel_id: the kernel wf_op_apply launches               */
  int plan_items, plan_patterns, plan_lz; /* lattice-column plan (WF_KERNEL_MARCH_IDX): work items,
                            distinct index tables, layers per item; 0 otherwise.  plan_lz of a box marching
                            operator: layers per z segment, or, when the whole apply runs by a run table
                            (wf_op_get_runs), the layers of its longest run */
  int plan_reoriented;   /* cells whose local axes the plan rotated / reflected to make them agree */
  double plan_fill;      /* cells / cell slots of the plan's columns                     */
  int geometry;          /* wf_geometry_mode of the stiffness geometry that was built    */
  int metric;            /* wf_metric_mode of the per-cell kernel, box or dofmap (0: none) */
  int update;            /* wf_update_mode of the separable kernel, box or dofmap (0: none); WF_UPDATE_ORDERED */
  int cell_coeff;        /* 1: created with a cell coefficient array (h_cell_coeff)      */
} wf_op_info_t;
int wf_op_info(const wf_op* op, wf_op_info_t* info); /* num_quads()/num_cells()/... mass.hpp:68-71 */

/* z segmentation of the box marching kernels (host only).  Work items run on `resident` workgroup slots, slot b mod nxcd
 * of XCD b mod nxcd, in launch order as slots free up; an item of L layers costs L + prologue.  The uniform plan cuts
 * every column into segments of *uniform_lz layers (the length that minimises rounds * (lz + 1.5) over equal cuts of at
 * least 3 layers; lz > 0: lz layers) and costs rounds * (*uniform_lz + prologue).  When a
 * plan of one run (column, z0, z1) per workgroup is strictly cheaper in this model, h_runs[3 r ..] receives run r in
 * launch order (runs r = k mod nxcd are XCD k's, every XCD a contiguous range of columns, longest run first) and *nruns
 * their number; otherwise *nruns = 0: the uniform plan stays.  It always stays for lz > 0 and when it needs one round
 * with its columns cut (or too short to cut: nz < 6).  capacity: runs h_runs can hold (ncols * nz always suffices). */
int wf_box_run_plan(int ncols, int nz, int resident, int nxcd, double prologue, int lz, int32_t* h_runs, int32_t capacity,
                    int32_t* nruns, double* cost, double* uniform_cost, int32_t* uniform_lz);
/* Box stiffness operator in the owner form (wf_op_info_t.update == WF_UPDATE_OWNER): plan wf_op_apply again.
 * resident > 0: by wf_box_run_plan for that many workgroups (a small mesh then takes a plan of many rounds).
 * resident = 0: as at creation, where a P4 operator without wf_tuning.lz whose uniform plan needs more than one round of
 * the resident workgroups times the uniform plan and cuts of every column at the same layers (4 to 12 layers per run)
 * on the device and keeps the fastest, and every other operator has no table.  Builds, replaces or drops the operator's
 * run table (counted in device_bytes); the interior / interface parts keep their z segments.  Synchronises the device.  wf_op_get_runs: the table, h_runs[3 r ..] = (column, z0, z1) of workgroup r, column = x piece +
 * pieces in x * y piece; *nruns = 0 without one (h_runs may be NULL to ask for the count). */
int wf_op_replan_runs(wf_op* op, int resident);
/* a caller's own table, checked to cover every layer of every column exactly once (nruns = 0: drop the table) */
int wf_op_set_runs(wf_op* op, const int32_t* h_runs, int32_t nruns);
int wf_op_get_runs(const wf_op* op, int32_t* h_runs, int32_t capacity, int32_t* nruns);
int wf_op_destroy(wf_op* op);

/* ---- cell forms: lambda^T A_c u per cell ----------------------------------------------------------
 * Not in the reference.  Every operator here is sum_c a_c P_c^T A_c P_c; a cell form evaluates
 *   e_c(lambda, u) = (P_c lambda)^T A^_c (P_c u),   one number per cell,
 * A^_c being the cell matrix the operator stores: for the stiffness operator with -c0^2, the -1/0/1 clamp and a_c, for
 * the lumped mass a_c det J w.  Without a coefficient e_c is d(lambda^T A u) / d a_c, the sensitivity kernel of an
 * adjoint-state inversion; with lambda = u it is the cell's share of the discrete energy.  One sum-factorised pass: the
 * geometry of an apply, two gathered vectors, one plain store per cell.
 *   Kinds     desc->kind = WF_OP_STIFFNESS or WF_OP_MASS_LUMPED; WF_OP_MASS_DENSE is WF_ERR_UNSUPPORTED.
 *   Set-up    that of wf_op_create: h_perm, WF_FLAG_TENSOR_X_SLOWEST, h_G / h_detJ or the mesh, WF_FLAG_NO_FABS,
 *             WF_FLAG_NO_CLAMP and h_cell_coeff (folded in once) mean what they mean there.  WF_FLAG_ORDERED and
 *             WF_FLAG_MASS_ELEMENTWISE are WF_ERR_INVALID: the form is order-fixed and element-wise by construction.
 *   Output    d_out [ncells] in the caller's cell order: the rows of h_dofmap; on a box cx + nx (cy + ny cz).
 *   Geometry  of the stiffness form: wf_tuning.geometry, the only tuning field that may be non-zero (any other is
 *             WF_ERR_INVALID).  AUTO: one G_c per cell (48 B, times a_c) when the mesh is given, h_G is NULL and every
 *             cell qualifies by the rule of wf_geometry_hex_cell; otherwise G per point.  PER_POINT forces G per point.
 *             PER_CELL is WF_ERR_INVALID for a cell that does not qualify (wf_last_error names the first) or without the
 *             mesh, and WF_ERR_UNSUPPORTED with h_G.  The lumped form ignores the field.
 *   Order     a thread sums its column (i, j, .) with k ascending, one thread sums the n^2 columns of its cell with
 *             j n + i ascending and stores out[c]: no atomics, bitwise reproducible; e_c depends neither on where the
 *             cell sits in the caller's order, nor on the other cells, nor on the launch.
 *   Checks    every argument check precedes the first device call.
 *   Streams   an evaluation holds no scratch state: any number of evaluations of one handle may be in flight on
 *             different streams.  d_lambda == d_u is allowed; d_out must not overlap either.
 *   Ranks     cells are rank-local and disjoint, so a partitioned mesh needs no exchange: the caller passes lambda and
 *             u with valid ghost entries and owns the cells it passes.
 *   alg_bytes stiffness ncells (48 nd | 48) + 4 nd ncells + 8 ncells + 16 ndofs; lumped ncells (12 nd + 8) + 16 ndofs. */
typedef struct wf_cell_form wf_cell_form;
typedef struct {
  int kind, degree, num_cells, ndofs;
  int geometry;          /* wf_geometry_mode of the stiffness form that was built; lumped: WF_GEOMETRY_AUTO */
  int cell_coeff;        /* 1: created with a cell coefficient array                                        */
  double alg_bytes;      /* algorithmic HBM bytes per evaluation                                            */
  size_t device_bytes;   /* device memory owned by the handle                                               */
} wf_cell_form_info_t;
int wf_cell_form_create(const wf_op_desc* desc, wf_cell_form** out);
int wf_cell_form_create_box(int kind, int degree, int nx, int ny, int nz, const double* h_xverts, double c0,
                            const double* h_cell_coeff, int flags, const wf_tuning* tuning, wf_cell_form** out);
/* out[c] = (accumulate ? out[c] : 0) + alpha * e_c(lambda, u), c = row of h_dofmap; d_lambda == d_u allowed */
int wf_cell_form_eval(const wf_cell_form* f, const double* d_lambda, const double* d_u, double alpha, int accumulate,
                      double* d_out, void* stream);
int wf_cell_form_info(const wf_cell_form* f, wf_cell_form_info_t* info);
int wf_cell_form_destroy(wf_cell_form* f);

/* ---- a8/a9: free kernels --------------------------------------------------
 * common/cuda/scatter.hpp:7-14, transform.hpp:7-8 (the reference passes a block
 * size; launch geometry is internal here). */
int wf_gather(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream);      /* out[i] = in[indices[i]]   */
int wf_scatter_add(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream); /* out[indices[i]] += in[i]  */
int wf_scatter_set(int32_t N, const int32_t* d_indices, const double* d_in, double* d_out, void* stream); /* out[indices[i]]  = in[i]  (VectorUpdater.hpp:141 unpack) */
int wf_transform1(int32_t N, const double* d_in, const double* d_detJ, double* d_out, void* stream);      /* out[i] = in[i]*detJ[i]    */

/* The two halves of the order-fixed accumulation as free functions.
 * wf_ordered_slots (host only): the plan of the order contract, a stable counting sort of the flattened dofmap.  The
 *   slots of dof d are h_row_off[d] .. h_row_off[d+1]-1; h_slot[c*nd + l] is the slot of entry (c, l), ascending with the
 *   position of the entry in h_dofmap.  WF_ERR_INVALID for an index outside [0, ndofs), WF_ERR_UNSUPPORTED if ncells*nd
 *   does not fit int32.
 * wf_segment_sum_add: y[d] = y[d] + (((vals[row_off[d]] + vals[row_off[d]+1]) + ...) + vals[row_off[d+1]-1]) for
 *   d < n, one thread per row, no atomics; rows of any length, an empty row leaves y[d] untouched; n = 0 is a no-op. */
int wf_ordered_slots(int64_t ncells, int nd, int32_t ndofs, const int32_t* h_dofmap, int32_t* h_row_off /*[ndofs+1]*/,
                     int32_t* h_slot /*[ncells*nd]*/);
int wf_segment_sum_add(int32_t n, const int32_t* d_row_off, const double* d_vals, double* d_y, void* stream);

/* ---- a12: tall-skinny dense matmul (TSMM) ---------------------------------
 * out[cell][n] = sum_k in[cell][k] * phi[k][n], phi row-major [K][N] on the device.
 * Replaces the cublasDgemm pair of demo/gpu_tsmm/main.cpp:49-52 and the B / B^T
 * products of demo/gpu_operator/main.cpp:149-155 (fp64 MFMA 16x16x4).
 * layout 0: in[cell*K + k], out[cell*N + n]   (cell-major, demo/gpu_operator)
 * layout 1: in[k*ncells + cell], out[n*ncells + cell]   (the column-major arrays
 *           of demo/gpu_tsmm with lda = ldc = ncells).
 * Any K, N > 0: columns run in passes of 128, table rows in ranges of <= 128 that
 * accumulate onto out (so out is read as well as written when K > 128). */
int wf_tsmm(int layout, int64_t ncells, int K, int N, const double* d_in, const double* d_phi, double* d_out,
            void* stream);

/* ---- a15/a16: vector kernels of the RK4 loop ------------------------------
 * common/LinearGLL.hpp:17-33 (copy, axpy), :173 (fill), :182-191 (divide),
 * common/cuda/la.hpp:31-138. */
int wf_copy(int64_t n, const double* d_in, double* d_out, void* stream);
int wf_fill(int64_t n, double value, double* d_out, void* stream);
int wf_axpy(int64_t n, double alpha, const double* d_x, const double* d_y, double* d_r, void* stream); /* r = alpha*x + y */
int wf_scale(int64_t n, double alpha, double* d_x, void* stream);
int wf_pointwise_div(int64_t n, const double* d_b, const double* d_m, double* d_out, void* stream);    /* out = b / m */
int wf_pointwise_mult_add(int64_t n, const double* d_m, const double* d_x, double* d_y, void* stream); /* y += m .* x */
int wf_dot(int64_t n, const double* d_x, const double* d_y, double* d_result, void* stream);           /* la.hpp:87 inner_product; result on device */

/* Fused vector algebra between two stiffness applies of the RK4 loop
 * (common/LinearGLL.hpp:182-191, :260, :264-265 and the next stage's :250-254):
 *   kv = b/m; ku = vn; u = ku*bdt + u_read; v = kv*bdt + v_read; b = 0 (LinearGLL.hpp:173);
 *   if has_next: un = ku*adt_next + u0; vn_next = kv*adt_next + v0.
 * u_read/v_read may alias u/v; vn_next must not alias vn. */
int wf_rk4_stage(int64_t n, double bdt, double adt_next, int has_next, double* d_b, const double* d_m,
                 const double* d_vn, const double* d_u_read, const double* d_v_read, double* d_u, double* d_v,
                 const double* d_u0, const double* d_v0, double* d_un, double* d_vn_next, void* stream);

/* ---- a7: boundary operator (diagonal form of forms.ufl:19-24) -------------
 * b[idx1[i]] += s1 * m1[i];  b[idx2[i]] += s2 * m2[i] * v[idx2[i]].
 * LinearGLL.hpp:175 with s1 = c0^2 g(t), s2 = -c0. */
int wf_boundary_apply(int32_t n1, const int32_t* d_idx1, const double* d_m1, double s1,
                      int32_t n2, const int32_t* d_idx2, const double* d_m2, double s2,
                      const double* d_v, double* d_b, void* stream);

/* The boundary term folded into the fused stage: a plan of the two boundary dof sets (host arrays, as
 * wf_boundary_apply takes them on the device) -- a bitmap over the n dofs, a running count per 64 dofs and
 * the facet masses of the union set in dof order.  wf_rk4_stage_bc is wf_rk4_stage that, instead of zeroing
 * b, leaves the NEXT right-hand side's boundary term in it:
 *   b[i] = s1_next m1[i] + s2 m2[i] v'[i],  v' = vn_next (has_next) or the updated v (last stage),
 * so the separate wf_boundary_apply launch per stage disappears (LinearGLL.hpp:173-175; the stiffness apply
 * then accumulates onto it).  wf_boundary_apply_plan is the plain launch (first right-hand side of a run). */
typedef struct wf_boundary wf_boundary;
int wf_boundary_create(int64_t n, int32_t n1, const int32_t* h_idx1, const double* h_m1, int32_t n2, const int32_t* h_idx2,
                       const double* h_m2, wf_boundary** out);
int wf_boundary_destroy(wf_boundary* bc);
int wf_boundary_apply_plan(const wf_boundary* bc, double s1, double s2, const double* d_v, double* d_b, void* stream);
int wf_rk4_stage_bc(int64_t n, double bdt, double adt_next, int has_next, double* d_b, const double* d_m,
                    const double* d_vn, const double* d_u_read, const double* d_v_read, double* d_u, double* d_v,
                    const double* d_u0, const double* d_v0, double* d_un, double* d_vn_next, const wf_boundary* bc,
                    double s1_next, double s2, void* stream);

/* Leapfrog (central difference, explicit Newmark beta = 0, gamma = 1/2) step of  m u'' + d u' - K u = s1 c1  with the
 * lumped mass m and the diagonal absorbing term d = -s2 c2 taken centred (implicit, at no cost: it is diagonal).
 * One stiffness apply and this one pass per step.  On entry d_b holds K u (the apply accumulated onto zeros, sign
 * convention of f1: u'' = b / m); with dt2 = dt*dt and hdt = (-s2)*(0.5*dt) computed by the host, per dof
 *   outside both boundary sets, and every dof of wf_leapfrog_step:
 *       a = b/m;  u_next = dt2*a + (2*u - u_prev)
 *   dof r of the plan's union set (c1, c2 the plan's facet masses, 0 where the dof is in one set only):
 *       h = hdt*c2[r];  u_next = (dt2*(b + s1*c1[r]) + ((2*m)*u - (m - h)*u_prev)) / (m + h)
 *   d_v non-null:  v = (u_next - u_prev) / (2*dt), the central velocity at the time of u
 *   b = +0.0 everywhere, ready for the next apply.
 * The expressions are evaluated as written (no fused multiply-add), so every compiled form gives the same bits.
 * d_u_next may be d_u_prev (in place); it must not overlap d_u, d_b or d_m, and d_v must not overlap any other
 * vector.  Refused (WF_ERR_INVALID, nothing written): a forbidden overlap, s2 > 0, dt <= 0, a plan built for another
 * n, a null vector or plan.  n <= 0 is a no-op.  48 B/dof of HBM traffic, 56 with d_v. */
int wf_leapfrog_step(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                     double* d_u_next, double* d_v, void* stream);
int wf_leapfrog_step_bc(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                        double* d_u_next, double* d_v, const wf_boundary* bc, double s1, double s2, void* stream);

/* The fourth-order leapfrog (modified-equation, "ME4") step: the two fused passes.  With A = M^-1 K (lumped mass m, sign
 * convention of f1: u'' = b / m) one step is
 *       (u+ - 2u + u-) / dt^2 = A u + (dt^2/12) A^2 u   (+ loads and their second difference),
 * fourth order in time, two stiffness applies and two passes per step, stable for dt <= sqrt(12) / sqrt(lambda_max(-A)):
 * sqrt(3) times the limit of wf_leapfrog_step.  The diagonal absorbing term d u', d = -s2 c2, is taken centred exactly
 * as wf_leapfrog_step_bc takes it and stays second order.
 *
 * One step, b = +0.0 on entry, dt2 = dt*dt, hdt = (-s2)*(0.5*dt), tdt = 2*dt, c12 = dt2/12 computed by the host:
 *   1. b += K u (the apply); wf_sources_add(t)
 *   2. wf_leapfrog4_predict, with s1 = s1(t):
 *        u_star = what wf_leapfrog_step_bc stores in u_next (the same expressions, the same bits)
 *        outside the plan's union set (and every dof without a plan):   w = c12*(b/m)
 *        dof r of the union set:                                         w = c12*((b + s1*c1[r])/m)
 *        b = +0.0
 *      d_u_star may be d_u_prev (in place); it must not overlap d_u, d_b, d_m or d_w; d_w overlaps no other vector.
 *      56 B/dof of HBM traffic.
 *   3. b += K w (the apply, ghost exchange as in 1)
 *   4. wf_sources_add_stencil at t - dt, t, t + dt with the weights 1/12, -2/12, 1/12 (the Numerov weighting of the load)
 *   5. wf_leapfrog4_correct, with s1c = (s1(t+dt) - 2*s1(t) + s1(t-dt))/12 from the host:
 *        outside the union set:   u_next = u_star + dt2*(b/m)
 *        dof r of the union set:  h = hdt*c2[r];  u_next = u_star + (dt2*(b + s1c*c1[r]))/(m + h)
 *        d_v non-null:            v = (u_next - u_prev)/tdt   (d_u_prev must then still hold u^{n-1}: step 2 out of place)
 *        b = +0.0
 *      d_u_next may be d_u_star (in place); it must not overlap d_b or d_m, nor d_u_prev when d_v is given; d_v overlaps
 *      no other vector.  d_u_prev is not read without d_v and may then be NULL.  40 B/dof, 56 with d_v.
 * The expressions are evaluated as written (no fused multiply-add), so every compiled form -- 16-byte and scalar sweep,
 * with and without a plan, with and without v -- gives the same bits.  bc may be NULL: no boundary sets (s1, s2 are then
 * not used, s2 is still checked).  Refused (WF_ERR_INVALID, nothing written): a forbidden overlap, s2 > 0, dt <= 0 or
 * NaN, a plan built for another n, a null vector.  n <= 0 is a no-op. */
int wf_leapfrog4_predict(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u, const double* d_u_prev,
                         double* d_u_star, double* d_w, const wf_boundary* bc, double s1, double s2, void* stream);
int wf_leapfrog4_correct(int64_t n, double dt, double* d_b, const double* d_m, const double* d_u_star, const double* d_u_prev,
                         double* d_u_next, double* d_v, const wf_boundary* bc, double s1c, double s2, void* stream);

/* ---- a14: ghost exchange over RCCL ----------------------------------------
 * demo/gpu_scatter_mpi/VectorUpdater.hpp:21-230 (GPU pack + CUDA-aware MPI per
 * IndexMap neighbour) and la::Vector::scatter_fwd / scatter_rev(add) of
 * common/LinearGLL.hpp:110,127,164-176.  One process per GPU; the transport is a
 * grouped ncclSend/ncclRecv per neighbour (RCCL over xGMI) enqueued on a HIP
 * stream -- no host synchronisation anywhere.  librccl is bound at run time.
 *
 * Communicator: rank 0 calls wf_comm_unique_id, the launcher distributes the 128
 * bytes (MPI_Bcast, torch.distributed, or the file rendezvous below), every rank
 * calls wf_comm_create after wf_set_device. */
#define WF_COMM_ID_BYTES 128
typedef struct wf_comm wf_comm;
typedef struct wf_updater wf_updater;
typedef enum { WF_SUM = 0, WF_MAX = 1 } wf_reduce_op;

int wf_comm_unique_id(char* id /* [WF_COMM_ID_BYTES] */);
int wf_comm_create(const char* id, int rank, int nranks, wf_comm** out);
/* rank 0 publishes the id in `path` (unique per job), the others poll up to timeout_s */
int wf_comm_rendezvous_file(const char* path, int rank, double timeout_s, char* id /* [WF_COMM_ID_BYTES] */);
int wf_comm_create_from_file(const char* path, int rank, int nranks, double timeout_s, wf_comm** out);
int wf_comm_info(const wf_comm* comm, int* rank, int* nranks, int* rccl_version); /* outputs may be NULL */
/* MPI_Allreduce of demo/gpu_cg/CUDA/cg.hpp:21 on device scalars / arrays (in place allowed) */
int wf_comm_allreduce(wf_comm* comm, int op, int64_t count, const double* d_in, double* d_out, void* stream);
int wf_comm_barrier(wf_comm* comm, void* stream);   /* all ranks reached this point; synchronises `stream` */
int wf_comm_destroy(wf_comm* comm);

/* The IndexMap data VectorUpdater's constructor reads (VectorUpdater.hpp:31-98).
 * Segment i of send_indices [send_offsets[i], send_offsets[i+1]) lists the OWNED
 * local dofs that send_neighbors[i] holds as ghosts (scatter_fwd_indices);
 * segment i of ghost_positions lists the local positions of the ghosts owned by
 * recv_neighbors[i] in the order that neighbour sends them.  Positions index the
 * whole local array (a DOLFINx caller passes size_local + ghost index).  A rank may
 * be its own neighbour (periodic partition). */
typedef enum {
  WF_UPDATER_DEFAULT = 0,
  WF_UPDATER_INLINE = 1   /* enqueue the exchange on the caller's stream instead of the
                             updater's communication stream (begin/end then do not overlap) */
} wf_updater_flags;       /* any other bit is refused (WF_ERR_INVALID) */
typedef struct {
  int ndofs;                          /* local array length: owned + ghosts               */
  int num_send_neighbors;
  const int* send_neighbors;          /* [num_send_neighbors] ranks                        */
  const int32_t* send_offsets;        /* [num_send_neighbors + 1], send_offsets[0] = 0     */
  const int32_t* send_indices;        /* [send_offsets[last]]                              */
  int num_recv_neighbors;
  const int* recv_neighbors;
  const int32_t* recv_offsets;        /* [num_recv_neighbors + 1]                          */
  const int32_t* ghost_positions;     /* [recv_offsets[last]]                              */
  int flags;                          /* wf_updater_flags                                  */
} wf_updater_desc;
int wf_updater_create(wf_comm* comm, const wf_updater_desc* desc, wf_updater** out);
/* update_fwd: owners -> ghosts (VectorUpdater.hpp:106-152).  begin packs on `stream`
 * and posts the exchange on the updater's own stream; work enqueued on `stream`
 * between begin and end overlaps with it; end makes `stream` wait and unpacks.
 * One exchange may be in flight per updater. */
int wf_updater_fwd_begin(wf_updater* u, const double* d_x, void* stream);
int wf_updater_fwd_end(wf_updater* u, double* d_x, void* stream);
int wf_updater_fwd(wf_updater* u, double* d_x, void* stream);
/* update_rev: ghosts -> owners, accumulating (VectorUpdater.hpp:157-208) */
int wf_updater_rev_begin(wf_updater* u, const double* d_x, void* stream);
int wf_updater_rev_end(wf_updater* u, double* d_x, void* stream);
int wf_updater_rev(wf_updater* u, double* d_x, void* stream);
int wf_updater_info(const wf_updater* u, int* num_send, int* num_recv, int* num_send_neighbors, int* num_recv_neighbors);
int wf_updater_destroy(wf_updater* u);

/* y += A x on a domain-decomposed mesh (LinearGLL.hpp:164-176 = scatter_fwd(x); apply;
 * scatter_rev(y)) with both halo directions hidden: update_fwd(x) -> apply(INTERFACE) ->
 * update_rev(y) runs on `stream` (the longer chain, so `stream` continues behind the reverse
 * unpack with no cross-stream wait on its critical path), apply(INTERIOR) beside it on a
 * low-priority stream of the updater; `stream` continues after both.
 * Needs wf_op_set_ghost_dofs / wf_op_set_ghost_faces. */
int wf_op_apply_overlapped(wf_op* op, wf_updater* u, double* d_x, double* d_y, void* stream);

/* ---- 8f: matrix-free conjugate gradients (BP1) -----------------------------
 * device::cg(x, b, matvec, kmax, rtol) of demo/gpu_cg/CUDA/cg.hpp:38-121: solves
 * A x = b for a symmetric positive definite operator, x holding the initial guess;
 * stops when ||r||^2 / ||r0||^2 < rtol^2 (cg.hpp:103) or after kmax iterations.
 * rtol = 0 runs kmax iterations unless the residual vanishes first (then its = k, res = 0).
 * A is an operator handle or a callback with the library's accumulate semantics
 * (y += A v; wf_cg zeroes y first).  On a partitioned mesh pass the updater and
 * its communicator: the halo of the direction is updated before, the product
 * accumulated to the owners after every matvec, and the reductions run over owned
 * entries with one scalar all-reduce each (the MPI_Allreduce of cg.hpp:15-24).
 * The textbook algorithm is implemented, not the reference loop's arithmetic
 * (update_rev(p), nrm2 used as a squared norm, axpy(1,p,r): cg.hpp:84,59,117).
 * Synchronises `stream`: the stopping test reads the residual on the host every
 * iteration, and iterations / rel_residual are host values on return. */
typedef int (*wf_matvec_fn)(void* user, const double* d_v, double* d_y, void* stream);
typedef struct {
  int64_t n;              /* local vector length (owned + ghost)                  */
  wf_op* op;              /* A; used when matvec is NULL                           */
  wf_matvec_fn matvec;    /* or a callback, y += A v                               */
  void* user;
  wf_updater* updater;    /* NULL on one rank                                       */
  wf_comm* comm;          /* NULL on one rank                                       */
  int kmax;               /* reference default 50                                   */
  double rtol;            /* reference default 1e-8                                 */
} wf_cg_desc;
int wf_cg(const wf_cg_desc* desc, double* d_x, const double* d_b, int* iterations, double* rel_residual, void* stream);

/* ---- 8f: mesh / facet-tag input (XDMF + HDF5) -------------------------------
 * demo/cpu_planar3d/main.cpp:39-45: io::XDMFFile("mesh.xdmf").read_mesh(element, ghost_mode,
 * "planar3d") and read_meshtags(mesh, "planar3d_boundaries").  Host-only; libhdf5 is bound
 * at run time.  Hexahedral meshes; vertex orders are converted to the engine's tensor order
 * (cells: v = a + 2b + 4c, facets: v = a + 2b).  Facet tags come back as the four vertices of
 * every tagged facet plus its value. */
typedef struct wf_mesh_file wf_mesh_file;
int wf_mesh_open(const char* xdmf_path, const char* grid_name, wf_mesh_file** out);
int wf_mesh_sizes(wf_mesh_file* m, int64_t* nverts, int64_t* ncells);
int wf_mesh_read(wf_mesh_file* m, double* h_xverts /* [nverts][3] */, int32_t* h_cells /* [ncells][8] */);
int wf_mesh_tags_size(wf_mesh_file* m, const char* tags_name, int64_t* nfacets);
int wf_mesh_read_tags(wf_mesh_file* m, const char* tags_name, int32_t* h_facet_verts /* [nfacets][4] */,
                      int32_t* h_values /* [nfacets] */);
int wf_mesh_close(wf_mesh_file* m);
/* writer in the same layout (tags_name may be NULL); <name>.xdmf + <name>.h5 */
int wf_mesh_write(const char* xdmf_path, const char* grid_name, int64_t nverts, const double* h_xverts, int64_t ncells,
                  const int32_t* h_cells, const char* tags_name, int64_t nfacets, const int32_t* h_facet_verts,
                  const int32_t* h_values);

/* ---- range markers (roctx) -----------------------------------------------------
 * The nvtxMarkA / cudaProfilerStart bracketing of demo/gpu_scatter_mpi/main.cpp:89,101-121.
 * wf_markers_enable(1) binds librocprofiler-sdk-roctx at run time; from then on wf_op_apply*,
 * wf_updater_*, wf_rk4_stage and wf_cg push / pop a named range on the calling host thread
 * (rocprofv3 --marker-trace).  Off by default; host code can add its own ranges. */
int wf_markers_enable(int on);
int wf_marker_push(const char* name);
int wf_marker_pop(void);
int wf_marker_mark(const char* name);

/* ---- 8f: what DOLFINx derives from the mesh for the CPU demo (host only) ------------------
 * demo/cpu_planar3d/main.cpp:39-66, common/LinearGLL.hpp:113-115.  Cells and facets in the
 * engine's tensor vertex order (wf_mesh_read / wf_mesh_read_tags deliver it); cells may have ANY
 * local orientation.
 * wf_fs_build: fem::create_functionspace(mesh, Lagrange(hexahedron, degree, gll_warped)): dofs are
 *   identified topologically (vertex / edge / face / interior entity + canonical position) and
 *   numbered in lexicographic (z, y, x) order of their coordinates.  h_dofmap [ncells][(P+1)^3],
 *   tensor order of each cell's own frame; h_dof_coords [coords_capacity >= *ndofs][3] may be NULL.
 * wf_fs_locate_facets: (cell, axis, side) of facets given by their four vertices (meshtags).
 * wf_fs_facet_mass: the tagged boundary dof set and its collocated facet masses
 *   m[i] = sum_facets w_q |dx/ds x dx/dt| (diagonal GLL form of forms.ufl:19-24), ascending dofs;
 *   h_idx / h_mass need capacity nfacets (P+1)^2.
 * wf_fs_min_cell_diameter: min over cells of mesh::h (largest vertex distance), main.cpp:48-57. */
int wf_fs_build(int degree, int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells,
                int64_t* ndofs, int32_t* h_dofmap, double* h_dof_coords, int64_t coords_capacity);
int wf_fs_locate_facets(int64_t ncells, const int32_t* h_cells, int64_t nfacets, const int32_t* h_facet_verts,
                        int32_t* h_cell, int32_t* h_axis, int32_t* h_side);
int wf_fs_facet_mass(int degree, int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells,
                     const int32_t* h_dofmap, int64_t nfacets, const int32_t* h_cell, const int32_t* h_axis,
                     const int32_t* h_side, int64_t* nout, int32_t* h_idx, double* h_mass);
/* wf_fs_facet_mass with every facet's contribution multiplied by h_cell_weight[cell of the facet] ([ncells], the
 * admittance 1/(rho c) of a heterogeneous medium); h_cell_weight = NULL is wf_fs_facet_mass. */
int wf_fs_facet_mass_weighted(int degree, int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells,
                              const int32_t* h_dofmap, int64_t nfacets, const int32_t* h_cell, const int32_t* h_axis,
                              const int32_t* h_side, const double* h_cell_weight, int64_t* nout, int32_t* h_idx,
                              double* h_mass);
int wf_fs_min_cell_diameter(int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells, double* hmin);

/* ---- the same for the box (host only) --------------------------------------------------------
 * mesh::create_box + fem::create_functionspace (demo/gpu_operator/main.cpp:60-72) on n[3] cells in this engine's
 * lexicographic numbering, and the Cartesian partition of a weak-scaled box (idea of demo/gpu_cg/mesh.hpp:37-63).
 * wavehip_box.hpp and the Python package are wrappers over these entries and hold no rule of their own.
 * wf_box_mesh: vertices h_x [nverts][3], vertex (a, b, c) -> a + (nx+1)(b + (ny+1)c) at lo + (hi-lo)/n * a, the last
 *   point exactly hi (numpy.linspace); h_geom_dofmap [ncells][8], vertex v = a + 2b + 4c of cell cx + nx (cy + ny cz).
 * wf_box_dofmap: h_dofmap [ncells][(P+1)^3], tensor order, dof (I, J, K) -> I + NX (J + NY K), NX = P nx + 1.
 * wf_box_facet_mass: wf_fs_facet_mass_weighted (the same loop) on the faces 2*axis + side whose face_tag equals tag
 *   (tag != 0; face_tag 0 = untagged), with the implicit dofmap: no array of ncells (P+1)^3 entries is needed.
 *   h_cell_weight [ncells] or NULL.  Ascending dofs.  With h_idx = h_mass = NULL only *nout is set; the arrays of the
 *   second call hold that many entries.
 * wf_decompose3d: nproc = px py pz with px >= py >= pz, the smallest (px - pz, px).
 * wf_box_partition: the part of rank `rank` of nproc = px py pz ranks, n[3] cells PER RANK, rank = rz + pz (ry + py rx).
 *   A lattice point shared by several ranks belongs to the lowest one, so a rank's ghosts are the lower planes of its
 *   local lattice where a lower neighbour exists; on a periodic axis (periodic[a] != 0; NULL = none) every rank's lower
 *   plane is ghost and the neighbours wrap (a rank can be its own neighbour).  Local vectors keep the lattice numbering.
 *   The lists are those of wf_updater_desc: neighbours ascending; the directions (dx, dy, dz) in {0,1}^3 that reach one
 *   neighbour are concatenated in loop order (dz fastest), on the sending and on the receiving side alike; inside a
 *   direction x runs fastest.  At most 7 neighbours each way: neighbour arrays of 7, offset arrays of 8 entries always
 *   suffice.  With all six arrays NULL only *info is filled (all six or none; the array of
 *   an empty index list may stay NULL). */
typedef struct {
  int procs[3], coords[3];
  int owned_lo[3];               /* first owned lattice index per axis (0 or 1)                     */
  int lattice[3];                /* local lattice (P n + 1 per axis), ghosts included                */
  int64_t size_global;           /* dofs of the whole box                                           */
  int64_t num_owned;
  int num_send_neighbors, num_recv_neighbors;
  int32_t num_send_indices, num_recv_indices;
  int face_tag[6];               /* cfg1: global face x = lo -> 1, other global faces -> 2, else 0  */
} wf_box_partition_info;
int wf_box_mesh(const int* n /* [3] */, const double* lo /* [3] */, const double* hi /* [3] */, double* h_x,
                int32_t* h_geom_dofmap);
int wf_box_dofmap(int degree, const int* n, int32_t* h_dofmap);
int wf_box_facet_mass(int degree, const int* n, const double* h_x, const int* face_tag /* [6] */, int tag,
                      const double* h_cell_weight, int64_t* nout, int32_t* h_idx, double* h_mass);
int wf_decompose3d(int nproc, int* procs /* [3] */);
int wf_box_partition(const int* n, int degree, int nproc, int rank, const int* periodic /* [3] */,
                     wf_box_partition_info* info, int* send_neighbors, int32_t* send_offsets, int32_t* send_indices,
                     int* recv_neighbors, int32_t* recv_offsets, int32_t* ghost_positions);

/* ---- point sources and receivers ---------------------------------------------------------------
 * Not in the reference (its only source is the plane term of Gamma_1, its only output a whole vector).
 *
 * Host, no device call (point_locate.cpp):
 * wf_points_locate: the cell and the reference coordinates of each of npoints physical points h_xyz [npoints][3] in
 *   the hexahedral mesh h_xverts [nverts][3], h_cells [ncells][8] (vertex v = a + 2b + 4c, as wf_geometry_hex).
 *   Reference coordinates are those of wf_tabulate_gll and wf_geometry_hex: xi in [0, 1]^3.  The trilinear map of the
 *   cell is inverted by Newton's method from the cell centre (at most 20 iterations); a cell accepts the point when
 *   the iteration converges and max |2 xi - 1| <= 1 + tol, i.e. every coordinate lies in [-tol/2, 1 + tol/2]; xi is
 *   then clamped to [0, 1].  A point on a face, edge or vertex shared by several cells goes to the LOWEST cell index.
 *   h_cell [npoints] receives the cell or -1 (in no cell: not an error of the call), h_ref [npoints][3] xi (0 there).
 *   Cells may be perturbed (non-affine) hexahedra.
 * wf_points_weights: h_w [npoints][3][P+1], the 1-D Lagrange basis on the GLL nodes of wf_tabulate_gll(P) at each
 *   reference coordinate, in barycentric form; a coordinate equal to a node (compared exactly) gives an exact 0/1 row.
 *   P outside 1..7: WF_ERR_UNSUPPORTED.
 * wf_sources_merge: the CSR wf_sources_create builds, for inspection: the unique dofs that nsrc point sources touch,
 *   ascending (h_dof [*nunique], h_off [*nunique + 1]); within a dof the sources ascending (h_src, h_weight
 *   [*nentries]).  h_dofs [nsrc][(P+1)^3], h_w [nsrc][3][P+1] are the rows of each source's point; the weight of entry
 *   l = i + n (j + n k) is (wx[i] * wy[j]) * wz[k]; entries whose weight is exactly zero are dropped.  Any output array
 *   may be NULL (the first call sizes the second).
 *
 * Device (points.hip):
 * wf_points_create: a set of points on a space of ndofs dofs.  h_dofs [npoints][nd], nd = (P+1)^3: the dofmap row of
 *   each point's cell in element-local tensor order l = i + n (j + n k); h_w as wf_points_weights writes it.  Indices
 *   outside [0, ndofs) are refused (WF_ERR_INVALID).
 * wf_points_sample: d_out[r] = sum_l (wx[i] wy[j]) wz[k] d_x[dofs[r][l]], l ascending per lane, lanes summed by a
 *   fixed butterfly: bitwise repeatable and independent of how many points are sampled together.  d_x holds ndofs
 *   entries; d_out holds npoints entries and may point anywhere inside a larger buffer.
 * wf_sources_create: nsrc point sources, source s at point h_point_of_source[s] of the plan, with wavelet
 *   h_wavelets[s].  A source is the right-hand side f = s(t) delta(x - x_s) of the equation as the model states it --
 *   u_tt - c0^2 Lap u = f, or (1/(rho c^2)) p_tt - div((1/rho) grad p) = f with a medium -- so its load is
 *   b[d] += s(t) phi_d(x_s).  The plan may be destroyed afterwards.
 *     WF_WAVELET_RICKER:  s(t) = amplitude (1 - 2a) e^{-a}, a = (pi frequency (t - delay))^2
 *     WF_WAVELET_SAMPLED: s(t) = amplitude times the linear interpolation of h_samples [nsamples] on t_start + k dt,
 *                         zero outside the table; nsamples >= 2, dt > 0
 * wf_sources_add: d_b[d] += sum over the sources at dof d, in source order, of weight * s(t): one thread and one
 *   update per unique dof, no atomics; the wavelets are evaluated on the device in fp64.
 * wf_sources_add_stencil: d_b[d] += sum over the sources at dof d, in source order, of weight * S,
 *   S = ((h_a[0] s(h_t[0])) + h_a[1] s(h_t[1])) + h_a[2] s(h_t[2])  (the first nt terms, 1 <= nt <= 3), one thread and one
 *   writer per dof like wf_sources_add; nt = 1 with h_a[0] = 1 gives the bits of wf_sources_add.  h_t and h_a are host
 *   arrays of nt doubles read during the call (they travel by value with the launch).  Refused: a null handle, nt outside
 *   1..3, a null array or vector, a time or weight that is not finite. */
typedef struct wf_points wf_points;
typedef struct wf_sources wf_sources;
enum { WF_WAVELET_RICKER = 0, WF_WAVELET_SAMPLED = 1 };
typedef struct {
  int kind;
  double amplitude, frequency, delay;
  int nsamples;
  const double* h_samples;
  double t_start, dt;
} wf_wavelet;
int wf_points_locate(int64_t nverts, const double* h_xverts, int64_t ncells, const int32_t* h_cells, int64_t npoints,
                     const double* h_xyz, double tol, int32_t* h_cell, double* h_ref);
int wf_points_weights(int P, int64_t npoints, const double* h_ref, double* h_w);
int wf_sources_merge(int P, int nsrc, const int32_t* h_dofs, const double* h_w, int32_t* nunique, int32_t* nentries,
                     int32_t* h_dof, int32_t* h_off, int32_t* h_src, double* h_weight);
int wf_points_create(int P, int64_t ndofs, int npoints, const int32_t* h_dofs, const double* h_w, wf_points** out);
int wf_points_destroy(wf_points* plan);
int wf_points_info(const wf_points* plan, int* npoints, int* nd, int* degree);
int wf_points_sample(const wf_points* plan, const double* d_x, double* d_out, void* stream);
int wf_sources_create(const wf_points* plan, int nsrc, const int32_t* h_point_of_source, const wf_wavelet* h_wavelets,
                      wf_sources** out);
int wf_sources_destroy(wf_sources* src);
int wf_sources_info(const wf_sources* src, int* nsources, int* nunique, int* nentries);
int wf_sources_add(const wf_sources* src, double t, double* d_b, void* stream);
int wf_sources_add_stencil(const wf_sources* src, int nt, const double* h_t, const double* h_a, double* d_b, void* stream);

/* ---- the passes of the discrete adjoint of the leapfrog loop (csrc/adjoint.hip) ----
 * wf_leapfrog_correlate: p[i] = p[i] + lam[i] * ((up[i] - 2.0*u[i]) + um[i]) for i < n, evaluated as written (no fused
 *   multiply-add), so every compiled form gives the same bits: the multiplier of a step times the second difference of
 *   the state, accumulated over the steps.  d_p must not overlap an input (WF_ERR_INVALID, nothing written); the inputs
 *   may overlap each other.  n <= 0 is a no-op.  48 B/dof of HBM traffic.
 * wf_sources_add_values: the wavelets are not looked at; d_values [nsources] on the device takes their place:
 *   acc = sum over the entries e of dof d, in the CSR order of wf_sources_merge, of weight[e] * d_values[source[e]];
 *   d_b[d] += scale * acc.  One thread and one update per unique dof, no atomics: with sources on the points of a
 *   wf_points plan it is the transpose of wf_points_sample.  d_values may point anywhere inside a larger buffer.
 *
 * The adjoint of the fourth-order loop (csrc/adjoint4.hip; notation of wf_leapfrog4_predict).  Step n of wf_wave_leapfrog4
 * is A+ u^{n+1} = dt2 K' u^n + 2 m u^n - A- u^{n-1} + loads with A+- = m +- h and K' = K + c12 K m^-1 K symmetric, so the
 * multipliers march backwards through the step itself:
 *       mu_N = mu_{N+1} = 0,   A+ mu_{k-1} = dt2 (K mu_k + K om_k + R^T r^k / dt) + 2 m mu_k - A- mu_{k+1},   om_k = c12 (K mu_k)/m,
 * wf_leapfrog4_predict on b = K mu_k with s1 = 0 (it leaves om_k in its w), the residual load onto b = K om_k AFTER the
 * predictor (before it, it would flow into om), wf_leapfrog4_correct with s1c = 0.  Per step n < N the sensitivities are
 *       stiffness cells:  dt2 (e_c(mu_n, u^n + w^n) + e_c(om_n, u^n))
 *       pointwise:        p += mu_n (u^{n+1} - 2 u^n + u^{n-1}) + 12 om_n w^n       (the second term: through the 1/m inside w)
 * with w^n the predictor's w of the forward step, and the mass sensitivity is the lumped-mass form of -p at the end.
 * wf_leapfrog4_correlate: for i < n
 *       p[i] = (p[i] + lam[i] * ((up[i] - 2.0*u[i]) + um[i])) + 12.0 * (om[i] * w[i])
 *       z[i] = u[i] + w[i]                                        (d_z may be NULL: no store)
 *   evaluated as written (no fused multiply-add), so the 16-byte and the scalar form of the sweep give the same bits.
 *   z is the right operand of the step's first cell form.  64 B/dof of HBM traffic, 72 with z.  Refused (WF_ERR_INVALID,
 *   nothing written): a null vector other than d_z; p or z overlapping an input or each other.  The inputs may overlap
 *   each other.  n <= 0 is a no-op. */
int wf_leapfrog_correlate(int64_t n, const double* d_lam, const double* d_up, const double* d_u, const double* d_um, double* d_p,
                          void* stream);
int wf_leapfrog4_correlate(int64_t n, const double* d_lam, const double* d_om, const double* d_up, const double* d_u,
                           const double* d_um, const double* d_w, double* d_p, double* d_z, void* stream);
int wf_sources_add_values(const wf_sources* src, const double* d_values, double scale, double* d_b, void* stream);

/* ---- the time loops of the wave model (csrc/wave_source.h, csrc/wave_loops.cpp; host code over the entries above) ----
 * The one copy of rk4_fused, leapfrog and leapfrog4: LinearGLLOpt of wave_fenics_amd/linear_gll.py and of wavehip_linear_gll.hpp
 * both call these.
 *
 * wf_wave_source: the plane source on Gamma_1 (LinearGLL.hpp:153-162).  c0_squared is the caller's own c0^2: the Python
 *   model forms c0 ** 2 (libm pow) and the C++ model c0 * c0, which differ in the last bit for about one speed in a
 *   thousand, and each keeps its bits.  With `medium` the facet masses carry the admittance and c0 is not read.
 *   wf_wave_window: the start-up ramp, 0.5 (1 - cos(freq0 pi t / alpha)) while t < period alpha, then 1.
 *   wf_wave_g: g(t) = window p0 w0 / c0 cos(w0 t), the Neumann datum without a medium.
 *   wf_wave_s1, wf_wave_s1_left_to_right: the coefficient of the Gamma_1 term in its two associations (wave_source.h);
 *   wf_wave_s2: the coefficient of the Gamma_2 term, -c0, or -1 with a medium.
 *
 * wf_wave_desc: what a loop works on.  The right-hand side b += K x is `rhs` when given (accumulate semantics, every
 *   launch on the stream it is handed), else the operator: wf_op_apply_overlapped(op, updater) when `overlapped`, else
 *   wf_updater_fwd(x) (with an updater), wf_op_apply, wf_updater_rev(b).  d_work points to wf_wave_work_vectors(scheme)
 *   device vectors of n doubles of the caller's, seven for WF_WAVE_RK4_FUSED, three for WF_WAVE_LEAPFROG and four for
 *   WF_WAVE_LEAPFROG4 (-1: an unknown scheme), distinct from each other and from every other vector of the call.  Their contents on entry do not matter.
 *   With receivers, row k of d_traces [trace_rows][npoints] receives u after step k (row 0: at t0) by wf_points_sample;
 *   h_times[k] (host, optional, with or without receivers) receives the time of that row.
 *
 * wf_wave_rk4_fused: RK4 (LinearGLL.hpp:198-287) from t0 while t < tf, the last step shortened to end at tf, with the
 *   vector algebra between two applies in one pass: per stage rhs, wf_rk4_stage_bc (fold_boundary; else wf_rk4_stage
 *   and wf_boundary_apply_plan), wf_sources_add.  s1 is wf_wave_s1_left_to_right at t + c_i dt.
 * wf_wave_leapfrog: central differences with a constant step (the last one is not shortened): a start-up apply for
 *   u^{-1}, per step rhs, wf_sources_add, wf_leapfrog_step_bc, and one finishing apply for the central velocity.  s1 is
 *   wf_wave_s1.  before_step (optional) is called before step k = 0, 1, ... with the time and the two states the step
 *   reads; d_a0 holds the start-up acceleration b / m at k = 0 only.  The loop's launches do not depend on it.
 * wf_wave_leapfrog4: the fourth-order loop (wf_leapfrog4_predict has the step), state (u, v) in and out as
 *   wf_wave_leapfrog, constant step, the last step not shortened, steps counted as wf_wave_step_count counts
 *   WF_WAVE_LEAPFROG; receivers record u at t0 and after every step.  Derivatives of the loads are central differences at
 *   t +- dt: the plane source through wf_boundary_apply_plan with the differenced s1 (wf_wave_s1), the point sources
 *   through wf_sources_add_stencil.
 *   Start-up (three applies): a0 = (K u0 + L(t0) - d v0)/m, j0 = (K v0 + L'(t0) - d a0)/m, q0 = (K a0 + L''(t0) - d j0)/m,
 *     u^{-1} = u0 - dt v0 + dt^2/2 a0 - dt^3/6 j0 + dt^4/24 q0.
 *   Finish (three applies): one more full step out of place gives vt = (u^{n+1} - u^{n-1})/(2 dt) and
 *     at = (u^{n+1} - 2 u^n + u^{n-1})/dt^2; then j = (K vt + L'(t) - d at)/m and v = vt - dt^2/6 j.  u is not advanced.
 *   A run split in two equals the continuous run to truncation order (the start-up is a Taylor series, not the inverse
 *   of the finish), not to rounding.
 *   before_step(user, n, t, u^{n-1}, u^n, d_startup ? d_startup[0] : NULL, stream) (optional) is called before step
 *   n = 0, 1, ... as wf_wave_leapfrog calls its own (not before the finishing step); it may copy the vectors, a non-zero
 *   return ends the loop with WF_ERR_INVALID.  d_startup, if not NULL, holds three vectors of n doubles that receive a0,
 *   j0 and q0 of the start-up (a copy after each is formed: the loop overwrites a0 with q0).  The loop's other launches
 *   and their order depend on neither.  Refused before the first launch: what wf_wave_leapfrog refuses, and a null entry
 *   of d_startup.
 * All three read the state d_u, d_v on entry and leave the result there; the forward ghost update of the result is the
 *   caller's.  max_steps < 0: no limit; otherwise the loop ends after the step that makes steps >= max_steps.  t_end and
 *   steps (host, optional) receive the time reached and the steps taken.  All launches go to `stream`; nothing is
 *   allocated, freed or synchronised.  Refused before the first launch (WF_ERR_INVALID): a null descriptor, state, work,
 *   m, b or plan, n < 0, neither op nor rhs, overlapped without an updater, receivers without d_traces, receivers or
 *   h_times with trace_rows < steps + 1, dt <= 0.
 * wf_wave_step_count: the steps a loop will take, by the loop's own t += dt accumulation (host only). */
typedef struct {
  double c0, c0_squared, p0, w0, freq0, alpha, period;
  int medium;
} wf_wave_source;
double wf_wave_window(const wf_wave_source* p, double t);
double wf_wave_g(const wf_wave_source* p, double t);
double wf_wave_s1(const wf_wave_source* p, double t);
double wf_wave_s1_left_to_right(const wf_wave_source* p, double t);
double wf_wave_s2(const wf_wave_source* p);

enum { WF_WAVE_RK4_FUSED = 0, WF_WAVE_LEAPFROG = 1, WF_WAVE_LEAPFROG4 = 2 };
typedef int (*wf_wave_rhs_fn)(void* user, double* d_x, double* d_b, void* stream);
typedef int (*wf_wave_step_fn)(void* user, int64_t step, double t, const double* d_u_prev, const double* d_u, const double* d_a0,
                               void* stream);
typedef struct {
  int64_t n;                     /* local vector length (owned + ghost)                                  */
  const double* d_m;             /* the lumped mass                                                      */
  double* d_b;                   /* the right-hand side vector                                           */
  const wf_boundary* bc;
  wf_wave_source source;
  int fold_boundary;             /* rk4_fused: the stage kernel leaves the next boundary term in b       */
  wf_op* op;                     /* K; used when rhs is NULL                                             */
  wf_updater* updater;           /* NULL on one rank                                                     */
  int overlapped;                /* wf_op_apply_overlapped (the operator is split)                       */
  wf_wave_rhs_fn rhs;            /* or a callback, b += K x with its ghost exchange                      */
  void* rhs_user;
  const wf_sources* sources;     /* optional                                                             */
  const wf_points* receivers;    /* optional                                                             */
  double* d_traces;
  double* h_times;               /* optional, host: the time of every row, [trace_rows]                  */
  int64_t trace_rows;
  double* const* d_work;         /* [wf_wave_work_vectors(scheme)] vectors of n doubles                  */
} wf_wave_desc;
int wf_wave_work_vectors(int scheme);
int64_t wf_wave_step_count(int scheme, double t0, double tf, double dt, int64_t max_steps);
int wf_wave_rk4_fused(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                      double* t_end, int64_t* steps, void* stream);
int wf_wave_leapfrog(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                     wf_wave_step_fn before_step, void* before_step_user, double* t_end, int64_t* steps, void* stream);
int wf_wave_leapfrog4(const wf_wave_desc* desc, double t0, double tf, double dt, int64_t max_steps, double* d_u, double* d_v,
                      wf_wave_step_fn before_step, void* before_step_user, double* const* d_startup, double* t_end,
                      int64_t* steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVEHIP_H */
