/* plfem.h — C-ABI of libplfem_hip.so: the MI355X (gfx950) implementation of the vectorial H-field
 * P2 FEM eigenmode path of KhaoulaAguech/pl-fem-vectoriel.
 *
 * The reference has no native boundary: the whole path is Python calling scikit-fem and SciPy
 * (reference solver_fem.py:113-239).  Each entry point below names the reference statement(s) it
 * replaces; the Python host (pl_fem_vectoriel_amd/solver_fem.py) binds them with ctypes and keeps
 * the reference's class / method surface.  INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - every function returns 0 on success and a negative PLFEM_E* code on failure; the message is
 *    available from plfem_last_error(ctx) (or the err buffer for the context-free symbolic calls);
 *    nothing throws across the boundary;
 *  - all array arguments are caller-owned; "host" / "dev" in a parameter name says where the
 *    pointer must live.  The library never frees caller memory;
 *  - DOF order of all full-length vectors is the reference's block order (solver_fem.py:166):
 *    x[0:N] = Hx DOFs, x[N:2N] = Hy DOFs, N = number of P2 DOFs including boundary DOFs, whose
 *    entries are kept at zero (Dirichlet H = 0, solver_fem.py:179-182); a context of the scalar solver
 *    (plfem_symbolic_create_ex with one unknown per node) has vectors of length N and, with dirichlet = 0, no
 *    eliminated DOFs -- wherever a size below says 2N / 2 nsolve it is dofs_per_node x N / nsolve;
 *  - all floating point data is IEEE double; indices are int32 (nnz < 2^31), offsets int64;
 *  - a plfem_ctx owns one HIP stream's worth of state; contexts are independent: the only process-wide
 *    state is two mutex-protected recycling pools (pinned staging blocks, timing events), so different
 *    contexts may be used from different threads; one context must not be used from two threads at once.
 */
#ifndef PLFEM_H
#define PLFEM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLFEM_OK 0
#define PLFEM_EINVAL (-1)   /* bad argument / inconsistent sizes            -> ValueError   */
#define PLFEM_EMESH (-2)    /* malformed mesh                               -> ValueError   */
#define PLFEM_EHIP (-3)     /* HIP runtime error (message has the call)     -> RuntimeError */
#define PLFEM_ENOCONV (-4)  /* Lanczos did not converge within maxiter      -> scipy ArpackNoConvergence */
#define PLFEM_ESTATE (-5)   /* call order violated (e.g. solve before factor) -> RuntimeError */
#define PLFEM_ESINGULAR (-6)/* factorisation broke down (sigma is an eigenvalue) -> RuntimeError */
#define PLFEM_ERESIDUAL (-7)/* plfem_solve_modes: eigenpairs fail the a-posteriori check even after the refined pass -> RuntimeError */
#define PLFEM_EHOST (-8)    /* host-side failure (out of memory, thread creation); the message has the cause -> RuntimeError */

typedef struct plfem_symbolic plfem_symbolic; /* host-only, mesh-only analysis               */
typedef struct plfem_ctx plfem_ctx;           /* device + stream + workspaces for one symbolic */

/* ---------------------------------------------------------------------------------------------
 * Symbolic phase (host, no GPU needed).
 * Replaces: Basis(mesh, ElementTriP2())            reference solver_fem.py:126
 *           basis.get_dofs().all() / setdiff1d     reference solver_fem.py:179-180
 *           sparsity work inside asm()/tocsr()     reference solver_fem.py:153-156
 *           splu ordering + symbolic factorisation scipy arpack.py:915 via solver_fem.py:197
 * p_host: [2][nv] doubles (x row, y row) = mesh.p; t_host: [3][ne] int32 = mesh.t.
 * leaf_elems: target triangles per leaf front of the nested-dissection tree (<=0: default).
 * ------------------------------------------------------------------------------------------- */
int plfem_symbolic_create(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                          int32_t leaf_elems, int32_t nthreads, plfem_symbolic** out,
                          char* err, int32_t errlen);
/* The same analysis for the scalar solver of the reference (ScalarHelmholtzSolver.solve, solver_fem.py:245-276,
 * SURVEY.md row f3): dofs_per_node = 1 (one unknown per P2 node; 2 = the vectorial H-field path) and
 * dirichlet = 0 (natural boundary: every node is kept, solver_fem.py:259 passes the full matrices to eigsh). */
int plfem_symbolic_create_ex(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                             int32_t leaf_elems, int32_t nthreads, int32_t dofs_per_node, int32_t dirichlet,
                             plfem_symbolic** out, char* err, int32_t errlen);
void plfem_symbolic_destroy(plfem_symbolic* sym);

/* info[] indices */
enum {
  PLFEM_INFO_NV = 0, PLFEM_INFO_NE, PLFEM_INFO_NEDGES, PLFEM_INFO_N, PLFEM_INFO_NSOLVE,
  PLFEM_INFO_NNZ, PLFEM_INFO_LEVELS, PLFEM_INFO_NFRONTS, PLFEM_INFO_FRONT_DOUBLES,
  PLFEM_INFO_MAX_FRONT, PLFEM_INFO_SOLVE_ENTRIES, PLFEM_INFO_FACTOR_FLOPS,
  PLFEM_INFO_T_NUMBERING_US, PLFEM_INFO_T_PATTERN_US, PLFEM_INFO_T_TREE_US, PLFEM_INFO_T_FRONTS_US,
  PLFEM_INFO_DOFS_PER_NODE, PLFEM_INFO_ARENA_DOUBLES, PLFEM_INFO_COUNT
};
int plfem_symbolic_info(const plfem_symbolic* sym, int64_t* info /* [PLFEM_INFO_COUNT] */);

/* Copy a named host array out of the analysis (for the Python compatibility surface and tests).
 * names: "edof"[6][ne] i32, "doflocs"[2][N] f64, "bmask"[N] u8, "interior"[nsolve] i32,
 * "rowptr"[N+1] i32, "colind"[nnz] i32, "slot_row"[nnz] i32, "nptr"[N+1] / "nadj"[6 ne] i32 / "nloc"[6 ne] u8
 * (node -> adjacent elements), "edges"[2][nedges] i32,
 * "leaf_of_elem"[ne] i32, "owner"[N] i32, "fs","fb"[nfronts] i32, "fnode_ptr","foff"[nfronts+1] i64, "soff"[nfronts] i64
 * (foff: kept part of a front = [F11; F21] m x s2 then Z^T s2 x b2; soff: its Schur complement inside the level's arena),
 * "fnodes","cinv0","cinv1"[fnode_ptr[nfronts]] i32, "epos"[6][ne] i32 (by element id), "epos_leaf"[ne][6] i32 (in the order of
 * "leaf_elems": what the device reads), "elem_nbr"[3][ne] i32 (the element across local edge (0,1), (1,2), (0,2), -1 on the
 * outer boundary; built on first request).
 * plfem_symbolic_array_bytes returns the size in bytes or a negative error. */
int64_t plfem_symbolic_array_bytes(const plfem_symbolic* sym, const char* name);
int plfem_symbolic_get(const plfem_symbolic* sym, const char* name, void* out_host, int64_t nbytes);

/* ---------------------------------------------------------------------------------------------
 * Mesh producer helper (the step before the path).
 * Replaces: MeshTri.refined() in MeshGenerator._generate_mesh   reference mesh.py:317-327
 * Uniform red refinement: new vertex id = nv + edge id (the P2 edge numbering), children
 * (t0,e0,e2), (t1,e0,e1), (t2,e2,e1), (e0,e1,e2), columns sorted.  p_out: [2][nv + nedges],
 * t_out: [3][4 ne]; nedges from plfem_mesh_edge_count.
 * ------------------------------------------------------------------------------------------- */
int plfem_mesh_edge_count(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                          int32_t* nedges, char* err, int32_t errlen);
int plfem_mesh_refine(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                      double* p_out, int32_t* t_out, char* err, int32_t errlen);

/* Marked refinement: longest-edge bisection with a conformity closure (host, stateless, deterministic); what an adaptive
 * loop refines the elements with that plfem_mode_indicators singles out.  marked_host[ne]: non-zero = refine this element.
 *   1. every marked element marks its longest edge -- squared lengths dx dx + dy dy from the sorted vertex pair of the
 *      edge (one value per edge, whichever element asks), ties to the smallest edge id;
 *   2. closure: an element with a marked edge also marks its own longest edge, until nothing changes;
 *   3. an element with 1 / 2 / 3 marked edges is bisected at its longest edge, then each child that holds another marked
 *      edge is bisected at that edge: 2 / 3 / 4 children.  The result is conforming.
 * Old vertices keep their ids; new vertex id = nv + the rank of its edge among the marked edges in edge-id order, at the
 * midpoint 0.5 (p_lo + p_hi); elements come out in the order of their parents, columns sorted; parent_out[ne_out] names
 * the parent.  plfem_mesh_refine_marked_count gives the sizes: p_out [2][nv_out], t_out [3][ne_out].
 * PLFEM_EINVAL (a null pointer) and PLFEM_EMESH (a mesh the numbering rejects) write their message to err. */
int plfem_mesh_refine_marked_count(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                                   const uint8_t* marked_host, int32_t* nv_out, int32_t* ne_out, char* err, int32_t errlen);
int plfem_mesh_refine_marked(int32_t nv, int32_t ne, const double* p_host, const int32_t* t_host,
                             const uint8_t* marked_host, double* p_out, int32_t* t_out, int32_t* parent_out,
                             char* err, int32_t errlen);

/* ---------------------------------------------------------------------------------------------
 * Context: binds a symbolic analysis to a device and stream, uploads the index structures and
 * allocates every workspace (nothing is allocated later, so calls are graph-capturable).
 * hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the default (null) stream.
 * max_ncv: largest Lanczos basis the context must hold, 3 <= max_ncv <= PLFEM_MAX_NCV.
 * Fails with PLFEM_EINVAL (message names the front order and the limit) when the largest front of the
 * analysis does not fit the solve sweeps' LDS staging even for one right-hand side (8 (m + 1) bytes of the
 * device's LDS per workgroup: ~20 000 DOFs on MI355X); between that and the limit for BLOCK_P = 4
 * right-hand sides (~5 000 DOFs) the eigen-solve silently uses the single-vector recurrence.
 * workspace_dev / workspace_bytes: optional caller-owned device memory (256-byte aligned, at least
 * plfem_workspace_bytes(sym, max_ncv) bytes, e.g. a torch tensor so that torch's caching allocator
 * recycles it between contexts) out of which EVERY device buffer of the context is carved; NULL / 0 =
 * the library hipMalloc's one slab itself and frees it in plfem_destroy.
 * plfem_create returns without synchronising: the one staged upload of the index structures (through a
 * pinned block from a small process-wide cache) and the pattern kernel are still in flight on the stream,
 * and every later call on the context is ordered behind them.  The symbolic handle must outlive the context.
 * ------------------------------------------------------------------------------------------- */
#define PLFEM_MAX_NCV 320
int plfem_workspace_bytes(const plfem_symbolic* sym, int32_t max_ncv, int64_t* bytes);
int plfem_create(const plfem_symbolic* sym, int32_t device, void* hip_stream, int32_t max_ncv,
                 void* workspace_dev, int64_t workspace_bytes, plfem_ctx** out, char* err, int32_t errlen);
void plfem_destroy(plfem_ctx* ctx);
const char* plfem_last_error(const plfem_ctx* ctx);
int plfem_synchronize(plfem_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * Numeric assembly.
 * Replaces: the nine @BilinearForm closures + 9 x asm()   reference solver_fem.py:131-156
 *           geometry.epsilon at quadrature points          reference geometry_unified.py:325-336
 *           block build A_xx..A_yy, B                      reference solver_fem.py:158-167
 * cores_host: [ncore][3] = cx, cy, r (closed discs, later cores overwrite earlier ones — with two
 * permittivities that is a union).  eps_core / eps_clad are n_core^2, n_clad^2 (the PML factor has
 * no real part contribution: solver_fem.py:132 takes np.real).  alpha_p is the divergence penalty
 * (solver_fem.py:158).  Fills the device CSR value arrays of the blocks
 * Axx, Axy, Ayx, Ayy, Minv (= B_xx = B_yy), Dxx, Dxy, Dyy on the shared scalar pattern.
 * ------------------------------------------------------------------------------------------- */
int plfem_assemble_hfield(plfem_ctx* ctx, const double* cores_host, int32_t ncore, double eps_core,
                          double eps_clad, double k0, double alpha_p);

/* Scalar Helmholtz pencil of the reference's ScalarHelmholtzSolver.solve, for a context whose
 * analysis has one unknown per node:
 * Replaces: stiff / mass_s / eps_m forms + 3 x asm() and K - k0^2 Me   reference solver_fem.py:251-259
 * Fills the AXX slot with K - k0^2 M_eps (the "A" of plfem_spmv / plfem_factor / plfem_lanczos_shift_invert /
 * plfem_residuals), the MINV slot with the plain mass matrix M (their "B"); all vectors then have length N. */
int plfem_assemble_scalar(plfem_ctx* ctx, const double* cores_host, int32_t ncore, double eps_core,
                          double eps_clad, double k0);

/* Index profile: a permittivity map beyond "discs of one eps_core on eps_clad" -- cladding plus jacket, trenches and
 * rings, graded cores, cores of unequal index.  A profile is a background permittivity eps_bg and an ordered table of
 * at most 64 layers of 8 doubles, layers_host[l][8] = (cx, cy, r_in, r_out, eps_a, eps_b, g, 0):
 *   membership: with dx = x - cx, dy = y - cy and d2 = fl(dx dx) + fl(dy dy), the point is in the layer when
 *     fl(r_in r_in) <= d2 <= fl(r_out r_out), every product rounded on its own (the arithmetic of the core test: a layer
 *     with r_in = 0 is the closed disc of plfem_assemble_hfield, ties included);
 *   value: g = 0: eps_a;  g > 0: eps_a + fl((eps_b - eps_a) t^g), t = (sqrt(d2) - r_in) / (r_out - r_in) clamped to
 *     [0, 1] (the alpha-profile n^2(rho) = n0^2 + (n_edge^2 - n0^2) (rho / a)^alpha);
 *   order: a later layer overwrites an earlier one; a point in no layer has eps_bg.
 * While a profile is set (nlayer > 0), plfem_assemble_hfield, plfem_assemble_scalar and plfem_solve_modes on this context
 * weigh every quadrature point with 1 / eps (the division made on the device, IEEE) -- eps in the scalar pencil -- of
 * the profile at the point as the assembly forms it, and do not read their eps_core / eps_clad.  Their cores argument
 * keeps its meaning: the discs the in-core sums of the post-processing count.  plfem_cmt_coupling does not read the
 * profile.  nlayer = 0 clears the profile: layers_host is not read, and eps_bg is kept as the background of an index map
(plfem_set_index_map) if it is finite and positive and is otherwise ignored, without an error.  The table is copied to a device
 * buffer of the context; the call synchronises the context's stream.
 * PLFEM_EINVAL, with the context's last error set: nlayer outside [0, 64]; a null table with nlayer > 0; a non-finite
 * entry or eps_bg; r_in < 0; r_out <= r_in; eps_a, eps_b or eps_bg <= 0; g < 0. */
int plfem_set_index_profile(plfem_ctx* ctx, const double* layers_host, int32_t nlayer, double eps_bg);

/* Sampled index map: the background of the profile as a pixel grid.  eps_host[j][i] (row-major, nx ny doubles) are
 * relative permittivities (n^2) on the uniform node grid x_i = x0 + i dx, y_j = y0 + j dy, 2 <= nx, ny <= 8192,
 * nx ny <= 2^24.  While a map is set, the permittivity of a point is
 *   inside the closed extent, 0 <= tx <= nx - 1 and 0 <= ty <= ny - 1 with tx = fl(fl(x - x0) fl(1 / dx)), ty likewise
 *     (false for a NaN): the bilinear interpolant of the map, formed as
 *       i0 = min(floor(tx), nx - 2), a = tx - i0, a1 = 1 - a;  j0, b, b1 likewise;
 *       lo = fl(a1 E[j0][i0]) + fl(a E[j0][i0+1]),  hi = fl(a1 E[j0+1][i0]) + fl(a E[j0+1][i0+1]),
 *       eps = fl(lo b1) + fl(hi b), every product rounded on its own (no fused multiply-add);
 *   outside it: eps_bg;
 * and the layers of plfem_set_index_profile are painted over that in their order.  The interpolant is bilinear in
 * eps = n^2, not in n.
 * While a map is set, plfem_assemble_hfield, plfem_assemble_scalar and plfem_solve_modes take the profile path even with
 * no layer set.  eps_bg is the one plfem_set_index_profile was last given: for a map without layers call
 * plfem_set_index_profile(ctx, NULL, 0, eps_bg), which sets no layer and keeps eps_bg (if it is finite and positive; any
 * other value is ignored, as before).  An assembly under a map with no such eps_bg is PLFEM_EINVAL.
 * A null map with nx = ny = 0 clears (the other arguments are not read).  The map is copied to a device buffer of the
 * context's own, outside its workspace, which is reused while it is large enough and freed by a clear and by
 * plfem_destroy; the call synchronises the context's stream.  With no map set every entry behaves, bit for bit, as it
 * did before this entry existed.
 * PLFEM_EINVAL, with the context's last error set and the context left as it was: nx or ny outside the limits; a null
 * map with non-zero sizes; a permittivity that is not finite or is <= 0; a non-finite origin; a step that is not finite,
 * is <= 0, or whose inverse is not finite. */
int plfem_set_index_map(plfem_ctx* ctx, const double* eps_host, int32_t nx, int32_t ny, double x0, double y0, double dx,
                        double dy);

/* Coupled-mode coupling integrals, scalar context only.
 * Replaces: the epsilon_product form + asm() and the E_i^H M_eps E_j loop of
 *           CoupledModeTheory._compute_rigorous_coupling                      reference config.py:296-320
 * M_deps = asm((Re eps - mean) u v), mean = plain mean of Re eps over ALL quadrature points (config.py:297-300; the
 * imaginary part is discarded by scikit-fem's float64 assembly); n real fields of length N each:
 * raw_host[i + j n] = E_i^T M_deps F_j with E = fields_i_dev[n][N], F = fields_j_dev[n][N]; pi/pj_host[i] = E_i.E_i, F_i.F_i.
 * The omega / 4 factor, the normalisation and the beta diagonal stay on the Python host as in the reference.
 * Overwrites the MINV slot: plfem_assemble_scalar must be called again before the next eigen-solve (PLFEM_ESTATE otherwise). */
int plfem_cmt_coupling(plfem_ctx* ctx, int32_t n, const double* fields_i_dev, const double* fields_j_dev,
                       const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                       double* raw_host, double* pi_host, double* pj_host, double* eps_mean_host);

enum { PLFEM_BLK_AXX = 0, PLFEM_BLK_AXY, PLFEM_BLK_AYX, PLFEM_BLK_AYY, PLFEM_BLK_MINV,
       PLFEM_BLK_DXX, PLFEM_BLK_DXY, PLFEM_BLK_DYY, PLFEM_BLK_COUNT };
/* device pointer of a block's CSR values (length nnz), valid until plfem_destroy */
int plfem_block_values_dev(plfem_ctx* ctx, int32_t block, const double** values_dev);
/* copy a block's CSR values to the host (synchronises the stream) */
int plfem_block_values_host(plfem_ctx* ctx, int32_t block, double* values_host);

/* ---------------------------------------------------------------------------------------------
 * CSR SpMV on the interior-restricted pencil, y = A_int x or y = B_int x embedded in 2N-vectors.
 * Replaces: B @ x inside ARPACK's reverse communication (scipy arpack.py:568-569) and the
 *           restriction A[idx,:][:,idx] (reference solver_fem.py:181-182) — boundary rows/cols masked.
 * which: 0 = A, 1 = B.
 * ------------------------------------------------------------------------------------------- */
int plfem_spmv(plfem_ctx* ctx, int32_t which, const double* x_dev, double* y_dev);

/* ---------------------------------------------------------------------------------------------
 * Shift-invert operator.
 * Replaces: splu((A - sigma B).tocsc())   scipy arpack.py:915 (via reference solver_fem.py:197)
 *           lu.solve(rhs)                 scipy arpack.py:920-928
 * Multifrontal block LDL^T factorisation (static pivoting: vanishing pivots are perturbed and counted,
 * plfem_timings()[5]) of the symmetric indefinite K = A_int - sigma B_int on the nested-dissection front
 * tree, all fronts dense in HBM, the unit-triangular pivot blocks inverted explicitly; solve = two sweeps
 * of batched dense panel products over the tree levels.  refine_steps extra iterative-refinement passes.
 * ------------------------------------------------------------------------------------------- */
int plfem_factor(plfem_ctx* ctx, double sigma);
int plfem_solve(plfem_ctx* ctx, const double* rhs_dev, double* x_dev, int32_t refine_steps);

/* ---------------------------------------------------------------------------------------------
 * Eigen-solve.
 * Replaces: eigsh(A_int, k, M=B_int, sigma=sigma, which='LM', tol, maxiter)
 *           reference solver_fem.py:196-197 -> scipy arpack.py:1359-1700 (mode 3, bmat='G').
 * Thick-restart Lanczos in the B inner product on OP = (A - sigma B)^-1 B with full (CGS2)
 * re-orthogonalisation; returns the k eigenvalues nearest sigma (largest |1/(lambda - sigma)|),
 * ascending, and B-orthonormal eigenvectors as 2N-vectors on the device.
 * Requires plfem_assemble_hfield + plfem_factor(sigma) before the call.
 * tol: a pair counts as converged when its Ritz residual ||r|| <= tol |theta|, theta = 1 / (lambda - sigma), the
 * criterion of ARPACK's dsaupd -- but tested after EVERY block step, and the iteration stops at the first step where
 * all k pairs meet it, where ARPACK tests at its restarts and usually ends orders of magnitude below its tolerance:
 * pass 1e-8 where the reference passes 1e-7 (measured agreement of the fields with eigsh: 3e-9 at 1e-8, 1e-7 at 1e-7).
 * evals_host[k]; evecs_dev[k][2N] (row c = vector c); stats_host[8] (may be NULL):
 *   [0] converged pairs, [1] OP applications, [2] restarts, [3] max relative Ritz residual.
 * stats_host[4] = passes over the factors (block solves; 0 = single-vector recurrence).
 * Returns PLFEM_ENOCONV if fewer than k pairs converged after maxiter RESTARTS of the basis (ARPACK
 * counts implicit restarts too: maxiter -> iparam[2] = mxiter, scipy arpack.py:358; outputs still hold the current Ritz pairs,
 * like ArpackNoConvergence.eigenvalues).  With the option "refine_steps" > 0 (plfem_set_option) every
 * OP application is followed by that many iterative-refinement passes r = Bx - K y, y += K^-1 r.
 * ------------------------------------------------------------------------------------------- */
int plfem_lanczos_shift_invert(plfem_ctx* ctx, int32_t k, int32_t ncv, double tol, int32_t maxiter,
                               double sigma, double* evals_host, double* evecs_dev, double* stats_host);

/* ---------------------------------------------------------------------------------------------
 * Per-mode post-processing.
 * Replaces: the per-mode loop of reference solver_fem.py:200-225 and _polarization_from_interp
 *           (solver_fem.py:68-107): Euclidean normalisation, divergence energy with the interior
 *           Dxx/Dxy/Dyy, core-mask sums.
 * evecs_dev[k][2N] as returned by plfem_lanczos_shift_invert (normalised IN PLACE to
 * sum(vx^2)+sum(vy^2) = 1 as solver_fem.py:213).  cores_host as in plfem_assemble_hfield.
 * out_host[k][PLFEM_POST_COUNT]; frac_core_host = (#interior DOF nodes inside a core)/N_solve.
 * modes_int_dev (may be NULL): [k][2*nsolve] interior-only copies (vx then vy) in the reference's
 * 'Ex_dofs'/'Ey_dofs' layout.
 * ------------------------------------------------------------------------------------------- */
enum { PLFEM_POST_NORM = 0, PLFEM_POST_DIV_ENERGY, PLFEM_POST_CORE_X, PLFEM_POST_CORE_Y,
       PLFEM_POST_ALL_X, PLFEM_POST_ALL_Y, PLFEM_POST_COUNT };
int plfem_postprocess(plfem_ctx* ctx, int32_t k, double* evecs_dev, const double* cores_host,
                      int32_t ncore, double* out_host, double* frac_core_host, double* modes_int_dev);

/* ---------------------------------------------------------------------------------------------
 * A-posteriori check of eigenpairs against the ASSEMBLED pencil (independent of the factorisation):
 * out_host[i] = || A v_i - lambda_i B v_i ||_2 / || A v_i ||_2 for the k vectors evecs_dev[k][2N].
 * No reference counterpart (eigsh trusts SuperLU's pivoting); here the LDL^T pivoting is static, so the
 * Python host checks every solve with this and re-runs with refinement when the check fails.
 * ------------------------------------------------------------------------------------------- */
int plfem_residuals(plfem_ctx* ctx, int32_t k, const double* evals_host, const double* evecs_dev, double* out_host);

/* ---------------------------------------------------------------------------------------------
 * The whole numeric solve in ONE call.
 * Replaces: everything TrueVectorialMaxwellSolver.solve_vectorial_modes does between the mesh analysis and its mode
 *           list -- assemble_hfield_system, the Dirichlet restriction, eigsh(..., sigma=...), the per-mode loop
 *           (reference solver_fem.py:176-225); on a scalar context ScalarHelmholtzSolver.solve (solver_fem.py:251-271).
 * = plfem_assemble_hfield (plfem_assemble_scalar on a context with one unknown per node) + plfem_factor(sigma) +
 *   plfem_lanczos_shift_invert(k, ncv, tol, maxiter) + plfem_postprocess + plfem_residuals, enqueued back to back on the
 *   context's stream, with the policy of the a-posteriori guard inside: if the largest residual exceeds residual_tol, or a
 *   vanishing pivot was perturbed, the eigen-solve is repeated with one more refinement pass inside the operator and the
 *   Ritz tolerance min(tol, tol_refined); if the check fails again: PLFEM_ERESIDUAL (message: plfem_last_error).
 * Behind the Lanczos iteration (which waits on its own step events) the host waits for the device ONCE; the copy of the
 * mode vectors to the host runs on a side stream beside the residual check.  Six C-ABI calls with four synchronisations
 * and the host work between them become one call: 0.3-0.5 ms of a 23-ms solve at C1.
 * Outputs (all caller-owned): evals_host[k] ascending; post_host[k][PLFEM_POST_COUNT] and *frac_core_host as
 * plfem_postprocess; resid_host[k] as plfem_residuals; modes_int_host (may be NULL): [k][dofs_per_node nsolve] interior
 * parts of the normalised vectors in the reference's 'Ex_dofs' / 'Ey_dofs' layout -- HOST memory, pinned for an
 * asynchronous copy (pageable memory works, synchronously); stats_host[PLFEM_SOLVE_STATS] (may be NULL), see the enum.
 * The full-length normalised vectors stay on the device in the context's own workspace: plfem_modes_dev.
 * PLFEM_ENOCONV: as plfem_lanczos_shift_invert (evals_host and plfem_modes_dev hold the current Ritz pairs).
 * ------------------------------------------------------------------------------------------- */
enum { PLFEM_SOLVE_NCONV = 0, PLFEM_SOLVE_NOPINV, PLFEM_SOLVE_RESTARTS, PLFEM_SOLVE_MAX_REL_RES, PLFEM_SOLVE_BLOCK_SOLVES,
       PLFEM_SOLVE_RESIDUAL_FIRST, PLFEM_SOLVE_RESIDUAL, PLFEM_SOLVE_REFINED, PLFEM_SOLVE_PERTURBED,
       PLFEM_SOLVE_T_ASSEMBLE_US, PLFEM_SOLVE_T_FACTOR_US, PLFEM_SOLVE_T_LANCZOS_US, PLFEM_SOLVE_T_POST_US,
       PLFEM_SOLVE_T_UPLOAD_US, PLFEM_SOLVE_T_RESIDUAL_US, PLFEM_SOLVE_T_CALL_US, PLFEM_SOLVE_STATS };
int plfem_solve_modes(plfem_ctx* ctx, const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                      double k0, double alpha_p, double sigma, int32_t k, int32_t ncv, double tol, int32_t maxiter,
                      double residual_tol, double tol_refined, double* evals_host, double* post_host,
                      double* frac_core_host, double* resid_host, double* modes_int_host, double* stats_host);
/* device pointer of the k full-length vectors ([k][dofs_per_node N], row c = vector c) the last plfem_solve_modes (or
 * plfem_lanczos_shift_invert) of the context produced; valid until the next plfem_factor / eigen-solve on the context */
int plfem_modes_dev(plfem_ctx* ctx, const double** evecs_dev, int32_t* k);

/* Options by name: "refine_steps" (iterative-refinement passes inside every OP application of
 * plfem_lanczos_shift_invert, default 0).  PLFEM_EINVAL for unknown names.  (No option alters a result in any other
 * way: the fault-injection hook of the test-suite is not in this library, see PLFEM_TEST_HOOKS below.) */
int plfem_set_option(plfem_ctx* ctx, const char* name, double value);

/* timings of the last calls in microseconds (HIP events on the context's stream):
 * [0] assemble, [1] factor, [2] lanczos, [3] postprocess, [4] upload; plus counters
 * [5] pivot perturbations in the last factorisation; [6] residual check of the last plfem_solve_modes. */
int plfem_timings(plfem_ctx* ctx, double* out_host /* [8] */);

/* ---------------------------------------------------------------------------------------------
 * Live timing for bench.py's "roofline" object (no reference counterpart): between begin and end
 * the ranges below are bracketed by HIP events on the context's stream.
 * out_host[PLFEM_PROF_COUNT][3] = { ranges timed, total microseconds, total algorithmic bytes } per slot:
 *   KFWD       every launch of the tile-form forward-sweep kernel (k_fwd, the largest single consumer
 *              of GPU time in a solve); algorithmic bytes of one launch = 8 B x sum over the level's fronts
 *              of (s2 m - s2^2/2 + P (m + s2)): the entries of [L11^-1 ; Z] read once + P staged / written vectors
 *   FWD_SWEEP  one whole forward sweep (all levels), same formula summed over all fronts
 *   BWD_SWEEP  one whole backward sweep
 *   SPMV_B     the block product B X of a Lanczos step: 12 B x nnz (Minv values + column indices of the
 *              shared pattern) + 4 B x (N + 1) row pointers + 2 x 8 B x P x 2N vector entries (read, written)
 * ------------------------------------------------------------------------------------------- */
enum { PLFEM_PROF_KFWD = 0, PLFEM_PROF_FWD_SWEEP, PLFEM_PROF_BWD_SWEEP, PLFEM_PROF_SPMV_B, PLFEM_PROF_COUNT };
int plfem_profile_begin(plfem_ctx* ctx, int32_t max_ranges);
int plfem_profile_end(plfem_ctx* ctx, double* out_host /* [PLFEM_PROF_COUNT][3] */);

/* ---------------------------------------------------------------------------------------------
 * Mode fields at arbitrary points and overlaps of modes across meshes (no solve context needed).
 * Replaces, on the user's side: scikit-fem Basis.probes(points) / Basis.interpolate(x) on the reference's
 *           Basis(mesh, ElementTriP2()) (reference solver_fem.py:126), and the integral of a field interpolated from
 *           one basis at the quadrature points of another (skfem Functional over basis_b with basis_a.interpolate);
 *           the reference itself evaluates no mode field anywhere.
 * A locator binds a symbolic analysis to a device and a stream: the point-location grid (built on the host on first
 * request, plfem_symbolic_get "loc_grid" [6] f64 = x0, y0, 1/hx, 1/hy, nx, ny; "loc_cell_ptr" [nx ny + 1] i32;
 * "loc_cell_elems" i32, ascending per cell; "loc_stats" [4] f64 = cells, mean / max candidates per cell, build seconds),
 * the vertex coordinates, element_dofs and the DOF -> interior map, uploaded into caller-owned device memory
 * (256-byte aligned, at least plfem_locator_bytes(sym) bytes; like plfem_create's workspace).  It allocates nothing
 * else, leaves plfem_workspace_bytes / plfem_create untouched, and the symbolic handle must outlive it.
 * Containment: a point is in element e when each of its three barycentric coordinates is >= -(PLFEM_LOC_TOL + the
 * rounding bound of that coordinate: PLFEM_LOC_EPS4 (|j11| (|x| + |x0|) + |j01| (|y| + |y0|)) / |det J| for xi, J = [p1-p0,
 * p2-p0]); a coordinate within its bound of 0 is set to 0 (the point is evaluated on that edge); among the
 * elements listed in the point's cell that contain it, the smallest element id wins; a point in none gets element -1
 * and value 0.
 * Mode layouts: "staged" = DOF-major, [ncomp][nrows][k] (plfem_stage_modes transposes [ncomp][k][nrows] into it);
 * indexed = 1: rows are interior DOFs (nrows = nsolve, the 'Ex_dofs' / 'Ey_dofs' layout), the map is int_index (a
 * boundary DOF contributes 0); indexed = 0: rows are all N DOFs ('field_vector' of the scalar solver).
 * ------------------------------------------------------------------------------------------- */
#define PLFEM_LOC_TOL 1e-10
#define PLFEM_LOC_EPS4 8.881784197001252e-16   /* 4 x DBL_EPSILON */
typedef struct plfem_locator plfem_locator;
int plfem_locator_bytes(const plfem_symbolic* sym, int64_t* bytes);
int plfem_locator_create(const plfem_symbolic* sym, int32_t device, void* hip_stream, void* mem_dev, int64_t mem_bytes,
                         plfem_locator** out, char* err, int32_t errlen);
void plfem_locator_destroy(plfem_locator* loc);
const char* plfem_locator_last_error(const plfem_locator* loc);
/* dst_dev[c][r][m] = src_dev[c][m][r] for c < ncomp, m < k, r < nrows (device, the locator's stream) */
int plfem_stage_modes(plfem_locator* loc, int32_t ncomp, int32_t k, int32_t nrows, const double* src_dev, double* dst_dev);
/* Sample k modes at npts points (device arrays, the locator's stream, no synchronisation).
 * ncomp = 1: out_dev[0][k][npts] = u; ncomp = 2: out_dev[0] = Hx, out_dev[1] = Hy, and with beta_dev (k doubles, or
 * NULL) out_dev[2] = Hz_im = -(dHx/dx + dHy/dy) / beta (the imaginary part of Hz under exp(j(wt - beta z))).
 * points_dev [2][npts] (x row, y row); elem_dev [npts]: the element each point was found in, or -1. */
int plfem_sample_fields(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                        const double* beta_dev, int32_t npts, const double* points_dev, double* out_dev, int32_t* elem_dev);
/* O[i][j] = sum over the elements of mesh B, over B's six-point rule (the assembly's), |det J| w_q wt(x_q) ua_i(x_q).ub_j(x_q)
 * (transverse dot product for ncomp = 2), ua located in mesh A inside the kernel.  wt = 1 when ncore < 0, else 1/eps(x)
 * with the closed-disc core test of plfem_assemble_hfield (ncore <= 64).  Partial ka x kb blocks per workgroup and a
 * fixed-order second stage: the same bits on every run.  work_dev: device scratch of plfem_overlap_work_bytes(ka, kb)
 * bytes; out_host [ka][kb] (synchronises the locators' stream; both locators on one device, loc_a's stream is used). */
int plfem_overlap_work_bytes(int32_t ka, int32_t kb, int64_t* bytes);
int plfem_field_overlap(plfem_locator* loc_a, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                        plfem_locator* loc_b, const double* modes_b_dev, int32_t kb, int32_t indexed_b, int32_t ncomp,
                        const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                        void* work_dev, int64_t work_bytes, double* out_host);
/* plfem_field_overlap under nposes poses of mesh A relative to mesh B, in one call.  A pose row is five doubles (tx, ty,
 * c, s, m): a point xi of mesh A appears in B's frame at x = t + m R xi, R = [[c, -s], [s, c]] (a shift, a rotation
 * and a magnification).  For B's quadrature point (X, Y), formed as the assembly forms it, A is located and evaluated at
 *   xa = (fl(c dx) + fl(s dy)) / m,  ya = (fl(c dy) - fl(s dx)) / m,  dx = X - tx, dy = Y - ty
 * (every product rounded on its own, the division IEEE: the identity pose (0, 0, 1, 0, 1) gives (X, Y) bit for bit and
 * the location decisions of plfem_field_overlap), and for ncomp = 2 A's value is turned into B's frame, (c ua_x - s ua_y,
 * s ua_x + c ua_y), before the dot product.  There is no amplitude factor for m: the self-overlap of the posed A is m^2
 * times its own.  out_host[p][i][j] = sum over the elements of B and B's six-point rule of |det J| w_q wt(x_q)
 * ua'_i(xa, ya) . ub_j(x_q); wt as in plfem_field_overlap, in B's frame; a point that lands in no element of A
 * contributes 0.
 * One workgroup per (slice of B's 64-point tiles, pair of 32-mode chunks, pose) writes its partial block to its own
 * slot, slices = min(128, tiles of B) whatever nposes, ka and kb are, and the fixed-order second stage of
 * plfem_field_overlap sums them: the bits of out_host[p] depend on pose p, the modes and the two meshes only -- not on
 * the other poses, on p's place in the table, on what the work buffer held or on the run.
 * The poses are worked off in batches of
 *   batch = max(1, min(nposes, 4096, (512 MiB - 768) / (8 (ka kb + 1024 pairs slices + 5)))) poses,
 * pairs = ceil(ka / 32) ceil(kb / 32) <= 256, and work_dev holds one batch: its results, its partial blocks and its
 * pose rows, each part 256-byte aligned, so plfem_overlap_posed_work_bytes(loc_b, ka, kb, nposes) never exceeds 512 MiB.
 * The pose rows travel to the device inside the work buffer.  Runs on loc_a's stream and synchronises it once, at the
 * end; both locators on one device.
 * Argument errors (nposes < 1, ka or kb < 1, more than 256 chunk pairs, ncomp not 1 or 2, ncore > 64, a null pointer,
 * work_bytes too small, a non-finite pose entry, m <= 0, |c^2 + s^2 - 1| > 1e-12) return PLFEM_EINVAL with loc_a's last
 * error set, before any launch. */
int plfem_overlap_posed_work_bytes(const plfem_locator* loc_b, int32_t ka, int32_t kb, int32_t nposes, int64_t* bytes);
int plfem_field_overlap_posed(plfem_locator* loc_a, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                              plfem_locator* loc_b, const double* modes_b_dev, int32_t kb, int32_t indexed_b, int32_t ncomp,
                              const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                              int32_t nposes, const double* poses_host /* [nposes][5] = tx, ty, c, s, m */,
                              void* work_dev, int64_t work_bytes, double* out_host /* [nposes][ka][kb] */);
/* Same-mesh Grams of k staged modes (indexed as for plfem_sample_fields) under the element forms of the assembly, over
 * the mesh's own six-point rule, split by the closed-disc core test of plfem_assemble_hfield (ncore in [0, 64]; r = core,
 * clad; every sum is over the points of region r of |det J| w_q (...)):
 *   ncomp = 2: out_host[0..4][k][k] = M_core, M_clad, K_core, K_clad, D with
 *     M_r[m][n] = sum_r hx_m hx_n + hy_m hy_n,
 *     K_r[m][n] = sum_r dy hx_m dy hx_n + dx hy_m dx hy_n - dx hx_m dy hy_n - dy hy_m dx hx_n  (the 1/eps-free part of
 *                 [[Kxx, Kxy], [Kyx, Kyy]]),
 *     D[m][n]   = sum dx hx_m dx hx_n + dy hy_m dy hy_n + dy hx_m dx hy_n + dx hy_m dy hx_n   ([[Dxx, Dxy], [Dxy^T, Dyy]]),
 *     so that V^T A V = sum_r K_r / eps_r + alpha_p D - k0^2 (M_core + M_clad) and V^T B V = sum_r M_r / eps_r;
 *   ncomp = 1: out_host[0..2][k][k] = M_core, M_clad, S (S[m][n] = sum grad u_m . grad u_n).
 * Partial blocks per workgroup and the fixed-order second stage of plfem_field_overlap: the same bits on every run.
 * work_dev: device scratch of plfem_gram_work_bytes(ncomp, k) bytes, 256-byte aligned; synchronises the locator's stream.
 * Argument errors (k <= 0, ncore outside [0, 64], a null pointer, work_bytes too small) return PLFEM_EINVAL with the
 * locator's last error set. */
int plfem_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_mode_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                     const double* cores_host, int32_t ncore, void* work_dev, int64_t work_bytes, double* out_host);

/* Grams of a profile solve: the forms of plfem_mode_grams with the permittivity of an index profile (layers_host, nlayer,
 * eps_bg as for plfem_set_index_profile; nlayer in [0, 64], eps_bg always read) in place of the two regions.  With
 * w = 1 / eps (ncomp = 2) or w = eps (ncomp = 1) of the profile at the quadrature point as the assembly forms it, every
 * sum over the six-point rule with |det J| w_q:
 *   ncomp = 2: out_host[0..3][k][k] = M, M_w, K_w, D with M[m][n] = sum hx_m hx_n + hy_m hy_n, M_w the same under w, K_w
 *     the form of K_r under w and D as in plfem_mode_grams, so that V^T A V = K_w + alpha_p D - k0^2 M, V^T B V = M_w;
 *   ncomp = 1: out_host[0..2][k][k] = M, M_w, S, so that V^T A V = S - k0^2 M_w, V^T B V = M.
 * Grid, tiling and second stage of plfem_mode_grams: the same bits on every run, for a subset or a permutation of the
 * modes, and whatever the work buffer held before.  The table is copied to a device buffer of the locator; synchronises
 * the locator's stream.
 * work_dev: device scratch of plfem_profile_gram_work_bytes(ncomp, k) bytes, 256-byte aligned: nout k^2 doubles plus
 * nout ceil(k / 32)^2 x 768 partial blocks of 8 KiB, nout = 4 or 3.
 * Argument errors (ncomp not 1 or 2, k < 1, a table plfem_set_index_profile rejects, eps_bg not finite and positive, a
 * null pointer, work_bytes too small) return PLFEM_EINVAL with the locator's last error set. */
int plfem_profile_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_profile_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                        const double* layers_host, int32_t nlayer, double eps_bg, void* work_dev, int64_t work_bytes,
                        double* out_host);

/* The sampled index map of plfem_set_index_map on a locator: while one is set, plfem_profile_grams evaluates its profile
 * over the map (eps_bg outside the extent, its layers painted over both), and plfem_mode_indicators takes its profile
 * path (layers_host, nlayer, eps_bg; the cores, eps_core and eps_clad are not read) even with nlayer = 0.  Both read
 * eps_bg from their own arguments, as before.  Arguments, model, clearing (a null map with nx = ny = 0) and argument
 * errors as for plfem_set_index_map, with the locator's last error set.  The map is copied to a device buffer of the
 * locator's own, outside the caller's memory, reused while it is large enough and freed by a clear and by
 * plfem_locator_destroy; the call synchronises the locator's stream. */
int plfem_locator_set_index_map(plfem_locator* loc, const double* eps_host, int32_t nx, int32_t ny, double x0, double y0,
                                double dx, double dy);

/* Per-core Grams: the Grams of k staged modes (staged and indexed as for plfem_mode_grams) over the quadrature points of
 * the mesh's own six-point rule that each core disc owns (ncore in [1, 64]; every sum is over the points of core c of
 * |det J| w_q (...)):
 *   ncomp = 2: out_host[c][0..2][k][k] = Mx, My, K with Mx[m][n] = sum_c hx_m hx_n, My[m][n] = sum_c hy_m hy_n and K the
 *     form of K_r of plfem_mode_grams; ncomp = 1: out_host[c][0][k][k] = M, M[m][n] = sum_c u_m u_n.
 * Ownership: a point belongs to the highest-index core whose closed disc holds it (the reference's epsilon lets later
 * cores overwrite earlier ones), decided with the arithmetic of the core test of plfem_assemble_hfield, so a point has
 * an owner exactly where that test puts it in the core: sum_c (Mx_c + My_c) = M_core and sum_c K_c = K_core of
 * plfem_mode_grams up to summation order.  Both pencils are linear in a per-region material constant, so with core c at
 * eps_c the projected pencil is V^T A V = sum_c K_c / eps_c + K_clad / eps_clad + alpha_p D - k0^2 M (vectorial; B
 * likewise from Mx_c + My_c) or S - k0^2 (sum_c eps_c M_c + eps_clad M_clad) (scalar).  count_host[c]: the quadrature
 * points core c owns; a core that owns none gives exact zeros.
 * Three passes: the owner of every point, per-core ascending point lists (counts, exclusive offsets, a stable fill: no
 * atomic decides a position), the Gram kernel over (slice, 32-mode chunk pair, core), then the fixed-order second stage
 * of plfem_field_overlap: the same bits on every run, whatever the work buffer held before.  Synchronises the
 * locator's stream.
 * work_dev: device scratch of plfem_core_gram_work_bytes(loc, ncomp, k, ncore) bytes, 256-byte aligned.  The bound, with
 * P = ceil(k / 32)^2 chunk pairs and nout = 3 or 1: slices = min(256, ceil(6 ne / 16), 1024 / ncore), at least 1 and the
 * same for every k (so that a subset of the modes gives the same bits), so the Gram kernel runs at most 1024 P
 * workgroups and the scratch is ncore nout k^2 doubles, at most 1024 nout P partial blocks of 8 KiB (24 MiB per chunk
 * pair for ncomp = 2: 24 MiB up to k = 32, 216 MiB at k = 70), and 2 x 6 ne + 128 int32.
 * Argument errors (ncomp not 1 or 2, k < 1, ncore outside [1, 64], a null pointer, work_bytes too small) return
 * PLFEM_EINVAL with the locator's last error set. */
int plfem_core_gram_work_bytes(const plfem_locator* loc, int32_t ncomp, int32_t k, int32_t ncore, int64_t* bytes);
int plfem_core_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                     const double* cores_host, int32_t ncore, void* work_dev, int64_t work_bytes,
                     double* out_host   /* [ncore][NOUT][k][k], NOUT = 3 (Mx, My, K) or 1 (M) */,
                     int64_t* count_host /* [ncore] quadrature points owned */);

/* Velocity Grams: the first-order change of the projected forms when the mesh moves with a velocity field and carries
 * its material along (the volume form of the shape derivative).  velocities_host [nvel][nv][2]: per
 * velocity a P1 field V on the mesh vertices, nvel in [1, 256].  Under x -> x + t V, every quadrature point keeping the
 * material it has, an element with the constant gradient G_ab = dV_a / dx_b, tr = G_xx + G_yy, changes
 *   grad f by -G^T grad f  ((G^T grad f)_b = sum_c G_cb d_c f)   and   |det J| w_q by tr |det J| w_q,
 * so with gt(f) = -G^T grad f + (tr / 2) grad f every gradient form changes by P + P^T, P[m][n] the form with gt on mode m
 * and the plain gradient on mode n, and every mass form by sum tr |det J| w_q c u_m . u_n.  For straight-sided P2 that is
 * the exact t-derivative of the discrete forms.  Modes staged and indexed as for plfem_mode_grams; the material
 * arguments are those of plfem_flux_grams (discs, a layer profile, or a profile over the locator's map), read at the
 * points of the unmoved mesh.  out_host[v][0..NOUT-1][k][k]:
 *   ncomp = 2: dK_w, dD, dM, dM_w -- K_w the form of K_r of plfem_mode_grams under w = 1 / eps, D, M = u . u', M_w under w --
 *     so that d(V^T A V) = dK_w + alpha_p dD - k0^2 dM and d(V^T B V) = dM_w;
 *   ncomp = 1: dS, dM, dM_w with w = eps, so that d(V^T A V) = dS - k0^2 dM_w and d(V^T B V) = dM.
 * count_host[v]: the elements with G != 0 (any of the four entries non-zero); the others contribute nothing, however large
 * V is there, and a velocity with none (zero, or a translation of everything) gives exact zeros and count 0.
 * Passes, per group of g velocities: G and the flag of every (velocity, element); per-velocity ascending element lists
 * (counts, exclusive offsets, a stable fill: no atomic decides a position); the Gram kernel over (slice of a list, 32-mode
 * chunk pair, velocity), which accumulates the asymmetric halves; the fixed-order second stage of plfem_field_overlap; and
 * X + X^T formed once per entry pair, so every matrix is bitwise symmetric.  The bits of out_host[v] depend on velocity v,
 * the modes, the material and the mesh only: not on the other velocities or v's place among them, on a subset or
 * permutation of the modes, on what the work buffer held, or on the run.  Synchronises the locator's stream.
 * work_dev: device scratch of plfem_velocity_gram_work_bytes(loc, ncomp, k, nvel) bytes, 256-byte aligned.  The bound, with
 * P = ceil(k / 32)^2 chunk pairs, nout = 4 or 3 and slices = min(128, ceil(6 ne / 16)) (at least 1; the same for every k
 * and nvel): a velocity takes nout P slices partial blocks of 8 KiB (4 MiB per chunk pair for ncomp = 2), and a group is
 * g = min(16, nvel, 256 MiB / that) velocities, at least 1 (16 up to k = 64, 7 at k = 70): at most 256 MiB of partial
 * blocks.  With the results, nvel nout k^2 doubles (38.3 MiB at nvel = 256, k = 70), and per group the velocities, flags and
 * lists of the mesh, g (16 nv + 8 ne) bytes, plus 128 bytes of counts, the scratch stays below 512 MiB for k <= 70 and any
 * nvel on meshes of up to about 800 000 elements.
 * Argument errors return PLFEM_EINVAL with the locator's last error set, before any launch, checked in this order: ncomp
 * not 1 or 2 or k < 1; nvel outside [1, 256]; ncore outside [0, 64]; a null array (cores only with ncore > 0); a non-finite
 * velocity entry; the material errors of plfem_flux_grams in its order; an indexed record on an analysis without interior
 * DOFs; work_bytes too small, then a misaligned buffer.  A null loc returns PLFEM_EINVAL alone.
 * plfem_velocity_gram_work_bytes rejects a null loc or bytes (left alone) and ncomp, k or nvel out of range. */
int plfem_velocity_gram_work_bytes(const plfem_locator* loc, int32_t ncomp, int32_t k, int32_t nvel, int64_t* bytes);
int plfem_velocity_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                         const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                         const double* layers_host, int32_t nlayer, double eps_bg, int32_t use_profile,
                         const double* velocities_host /* [nvel][nv][2] */, int32_t nvel,
                         void* work_dev, int64_t work_bytes,
                         double* out_host    /* [nvel][NOUT][k][k], NOUT = 4 (dK_w, dD, dM, dM_w) or 3 (dS, dM, dM_w) */,
                         int64_t* count_host /* [nvel] elements with a non-zero velocity gradient */);

/* Coordinate-weighted ("moment") Grams: the region Grams of plfem_mode_grams weighted by the coordinates of the
 * quadrature point, X = x - origin_host[0], Y = y - origin_host[1], (x, y) the physical point exactly as the assembly
 * forms it; modes, indexed, cores and regions as for plfem_mode_grams (ncore in [0, 64]); every sum is over the six-point
 * rule with |det J| w_q:
 *   ncomp = 1: out_host[0..6][k][k] = M_core_X, M_core_Y, M_clad_X, M_clad_Y, M_XX, M_XY, M_YY with
 *     M_r_X[m][n] = sum_r X u_m u_n (likewise Y), M_XX[m][n] = sum X^2 u_m u_n over both regions (likewise XY, Y^2);
 *   ncomp = 2: out_host[0..10][k][k] = M_core_X, M_core_Y, M_clad_X, M_clad_Y, K_core_X, K_core_Y, K_clad_X, K_clad_Y,
 *     M_XX, M_XY, M_YY with M = hx hx' + hy hy' and K the form of K_r of plfem_mode_grams.
 * A bend of curvature kappa along (c, s) enters both pencils linearly -- eps -> eps (1 + 2 kappa (c X + s Y)) in the
 * scalar form, 1/eps -> (1 - 2 kappa (c X + s Y)) / eps in the vectorial form -- so these are the exact projections of
 * the bent pencils on the span of the modes; the second moments give centroids and widths.
 * The grid and tiling of plfem_mode_grams (the tile-to-workgroup map does not depend on k), partial blocks per
 * workgroup, every one written by the call that reads it, and the fixed-order second stage: the same bits on every run,
 * for a subset or a permutation of the modes, and whatever the work buffer held before.  Synchronises the locator's
 * stream.
 * work_dev: device scratch of plfem_moment_gram_work_bytes(ncomp, k) bytes, 256-byte aligned: nout k^2 doubles plus
 * nout ceil(k / 32)^2 x 768 partial blocks of 8 KiB, nout = 7 or 11 (66 MiB for ncomp = 2 up to k = 32, 594 MiB at k = 70).
 * Argument errors (ncomp not 1 or 2, k < 1, ncore outside [0, 64], a null pointer, a non-finite origin, work_bytes too
 * small) return PLFEM_EINVAL with the locator's last error set. */
int plfem_moment_gram_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_moment_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                       const double* cores_host, int32_t ncore, const double origin_host[2], void* work_dev,
                       int64_t work_bytes, double* out_host);

/* Tangent Grams of a profile solve: the M_w (and K_w) of plfem_profile_grams under a batch of point weights ("columns")
 * in place of w.  Modes, indexed, layers_host, nlayer, eps_bg and the locator's sampled map as for plfem_profile_grams.
 * Both pencils are linear in the VALUES of the profile at fixed shapes (eps_bg, eps_a and eps_b of every layer, every
 * pixel of the map), so a first-order change of those values -- a tangent -- is a profile with the same layers and the
 * same grid: tangents_host[t] = (d_eps_bg, then (d_eps_a, d_eps_b) of every layer), and optionally a map of d eps on the
 * locator's map grid, tangent_maps_host[tangent_map_host[t]] (tangent_map_host may be null when nmap = 0; nmap > 0 needs
 * a map on the locator).  At a quadrature point, as the assembly forms it, d eps_t is d_eps_a + (d_eps_b - d_eps_a) t^g in
 * the topmost layer that holds the point (d_eps_a for a constant layer: g = 0; membership, t and g of the profile);
 * otherwise, inside the closed extent of the locator's map, the bilinear interpolant of the tangent's map -- or
 * tangents[t][0] if it has none --; otherwise tangents[t][0].  With w = 1 / eps (ncomp = 2) or w = eps (ncomp = 1) formed
 * as plfem_profile_grams forms it, column t < ntan has the point weight dw_t = -(d eps_t w) w (ncomp = 2) or d eps_t
 * (ncomp = 1); with moments != 0 two more columns follow, w X and w Y, X = x - origin_host[0], Y = y - origin_host[1]
 * (origin_host is always read).  Every sum over the six-point rule with |det J| w_q and the column's weight c:
 *   ncomp = 2: out_host[col][0..1][k][k] = M_col, K_col with M_col[m][n] = sum c (hx_m hx_n + hy_m hy_n) and K_col the
 *     form of K_r of plfem_mode_grams under c: d(V^T B V) = M_col and d(V^T A V) = K_col along tangent col; a bend of
 *     curvature kappa along X moves the pencil by -2 kappa (K_wX, M_wX);
 *   ncomp = 1: out_host[col][0][k][k] = M_col: d(V^T A V) = -k0^2 M_col, and -2 kappa k0^2 M_wX for a bend.
 * The unweighted moments (centroids, widths) carry no material: plfem_moment_grams with ncore = 0 has them.
 * Columns go in groups of 4.  Per group: a pre-pass with one lane per quadrature point walks the layer table once, forms
 * w and writes the group's four weights of the point; a Gram kernel with the grid and tiling of plfem_mode_grams forms
 * the unweighted products m = u . u' and kk (the form of K_r) of a point once and adds them, times each column's
 * weight, to that column's partial blocks; the fixed-order second stage of plfem_field_overlap sums them.  The same bits
 * on every run, for a subset or a permutation of the modes, whatever the work buffer held before, and for a column
 * whatever other columns share the call and however they fall into groups.  Synchronises the locator's stream.
 * work_dev: device scratch of plfem_profile_tangent_gram_work_bytes(loc, ncomp, k, ntan, nmap, moments) bytes, 256-byte
 * aligned, every part rounded up to 256 bytes: the result, ncol nout k^2 doubles (ncol = ntan + 2 for moments, nout = 2 or
 * 1); the partials of one group, 4 nout ceil(k / 32)^2 x 768 blocks of 8 KiB (48 MiB for ncomp = 2 up to k = 32, 432 MiB at
 * k = 70); 4 x 6 ne point weights; ntan x 129 doubles of tangent rows; ntan int32; nmap nx ny doubles of tangent maps (the
 * locator's grid), the last three at least one entry each.  So bytes <= 8 (ncol nout k^2 + 4 nout ceil(k / 32)^2 786432 +
 * 24 ne + 129 max(ntan, 1) + max(nmap nx ny, 1)) + 4 max(ntan, 1) + 6 x 256.
 * Argument errors (ncomp not 1 or 2, k < 1, ntan outside [0, 256], ntan + 2 moments < 1, nmap outside [0, min(ntan, 8)],
 * nmap > 0 without a map on the locator, a table plfem_set_index_profile rejects, a null pointer, a map index outside
 * [-1, nmap), a tangent entry or an origin that is not finite, work_bytes too small) return PLFEM_EINVAL with the
 * locator's last error set. */
int plfem_profile_tangent_gram_work_bytes(const plfem_locator* loc, int32_t ncomp, int32_t k, int32_t ntan, int32_t nmap,
                                          int32_t moments, int64_t* bytes);
int plfem_profile_tangent_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                                const double* layers_host, int32_t nlayer, double eps_bg,
                                const double* tangents_host /* [ntan][1 + 2 nlayer] */, int32_t ntan,
                                const double* tangent_maps_host /* [nmap][ny][nx] or NULL */, int32_t nmap,
                                const int32_t* tangent_map_host /* [ntan]: index into the maps, or -1 */,
                                int32_t moments, const double origin_host[2],
                                void* work_dev, int64_t work_bytes, double* out_host);

/* Pixel densities of a sampled map: the derivative of the diagonal of M_w (and K_w) of plfem_profile_grams in the value
 * of EVERY pixel of the locator's map E[ny][nx] (plfem_locator_set_index_map), in one pass over the quadrature points
 * whatever the number of pixels -- the adjoint of the bilinear interpolant of the profile.  Modes, indexed, layers_host,
 * nlayer and eps_bg as for plfem_profile_grams; the staged fields v_r are the modes or any combination of them formed
 * before staging.  At a point of the six-point rule, formed as the assembly forms it: the topmost layer, the map cell
 * (i0, j0) and the weights (a, b), eps and w = 1 / eps (ncomp = 2) or eps (ncomp = 1) as plfem_profile_tangent_grams forms
 * them.  The point CONTRIBUTES when it lies in the closed extent of the map and no layer holds it.  It then adds
 * c = |det J| w_q dw, dw = -(w w) (ncomp = 2) or 1 (ncomp = 1), times a density of the field, times the corner weight
 * a1 b1, a b1, a1 b, a b (a1 = 1 - a, b1 = 1 - b) to the nodes (j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1); the
 * clamped cell of the last column (i0 = nx - 2, a = 1) feeds column nx - 1.  Densities and outputs:
 *   ncomp = 2: m_r = hx_r^2 + hy_r^2 and kk_r = the form of K_r of plfem_mode_grams at m = n, (dy hx)^2 + (dx hy)^2 -
 *     2 dx hx dy hy; out_host[r][0] = M_px[r] = d(v_r^T B v_r) / dE and out_host[r][1] = K_px[r] = d(v_r^T A v_r) / dE;
 *   ncomp = 1: m_r = u_r^2; out_host[r][0] = M_px[r] = d(M_w)_rr / dE, so d(v_r^T A v_r) / dE = -k0^2 M_px[r].
 * So for any tangent map D on the grid sum_ji D[j][i] M_px[r][j][i] = M_d[r][r] of plfem_profile_tangent_grams for the
 * tangent (0, 0.., map D), K likewise.  support_host[j][i] (may be null) = the number of contributing points in the up
 * to four cells the node is a corner of; a node with support 0 carries an exact 0 in every plane (the mesh does not see
 * the pixel, or layers cover it).
 * Kernels: one lane per point writes the point's cell as a key (one past the last cell where it does not contribute)
 * with (a, b, c); a stable radix sort of (key, point) on 25 bits makes every cell's points contiguous in ascending point
 * order; per chunk of 16 fields one lane per contributing point writes the densities, and one wavefront per node with a
 * non-empty list walks the node's cells in ascending order, lane l taking every 64th point from the l-th, and sums the
 * lanes by a fixed butterfly.  No floating-point atomics: the same bits on every run, for a field whatever other fields
 * share the call and in whatever order, and whatever the work buffer held.  Every entry of out_host and support_host is
 * written.  Synchronises the locator's stream.
 * work_dev: device scratch of plfem_index_map_gradient_work_bytes(loc, ncomp, k) bytes (it depends on the mesh and on the
 * map, hence the locator), 256-byte aligned, every part rounded up to 256 bytes: k nout nx ny doubles of result (nout = 2
 * or 1); nx ny int32; 4 x 6 ne uint32 and 3 x 6 ne doubles of keys and point data; 16 nout x 6 ne doubles of densities;
 * 2 (nx - 1)(ny - 1) int32 of cell ranges; the sort's temporary storage (about 2 x 6 ne uint32 plus its histograms).
 * Argument errors (ncomp not 1 or 2, k outside [1, 256], no map on the locator, k nout nx ny > 2^27 -- 1 GiB of result:
 * call with fewer fields --, a table plfem_set_index_profile rejects, a null modes_dev, work_dev or out_host, work_bytes
 * too small) return PLFEM_EINVAL with the locator's last error set and nothing written.
 * plfem_index_map_gradient_work_bytes rejects a null loc or bytes (left alone) and the first four of these; the sort's
 * storage is sized by rocPRIM for the device at hand, so without a device it returns PLFEM_EHIP. */
int plfem_index_map_gradient_work_bytes(const plfem_locator* loc, int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_index_map_gradients(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                              const double* layers_host, int32_t nlayer, double eps_bg,
                              void* work_dev, int64_t work_bytes,
                              double* out_host /* [k][nout][ny][nx], nout = 2 (M_px, K_px) or 1 */,
                              int32_t* support_host /* [ny][nx] or NULL */);

/* Quartic mode-overlap tensor of k staged modes over the locator's mesh (the input of multimode nonlinear propagation:
 * f_ijkl, A_eff, gamma), on the 16-point degree-8 rule (products of four P2 fields are of degree 8).  Pairs i <= j are
 * numbered p(i,j) = i k - i (i - 1) / 2 + (j - i), np = k (k + 1) / 2.
 *   out_host[p(i,j)][p(l,m)] = sum over the elements and the 16 points of |det J| w_q wt(x_q) (u_i . u_j)(u_l . u_m),
 * np x np, exactly symmetric (one triangle computed, mirrored); u . u' = hx hx' + hy hy' when ncomp = 2.  wt = 1 when
 * ncore < 0, otherwise w_core / w_clad by the assembly's closed-disc core test (cores_host = (x, y, r) per core).
 * modes_dev: staged by plfem_stage_modes ([ncomp][nrows][k]); indexed as in plfem_sample_fields.  Partial tiles per
 * workgroup and a fixed-order second stage: the same bits on every run.  Synchronises the locator's stream.
 * work_dev: device scratch of plfem_quartic_work_bytes(ncomp, k) bytes, 256-byte aligned.  The bound: np x np doubles
 * for the result plus at most 2048 partial 64 x 64 tiles, so at most 34.6 MB + 67.1 MB (k = 64); 42 MB at k = 22.
 * Argument errors (ncomp not 1 or 2, k outside [1, 64], ncore > 64, a null pointer, work_bytes too small) return
 * PLFEM_EINVAL with the locator's last error set. */
int plfem_quartic_work_bytes(int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_mode_quartic(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                       const double* cores_host, int32_t ncore, double w_core, double w_clad,
                       void* work_dev, int64_t work_bytes, double* out_host);

/* Projection of k staged modes on a family of analytic fields that separate in x and y: plane waves (far field) and
 * Gaussian beams of any centre, waist and tilt (launch maps).  A factor is a triple (c, s, kappa) of finite doubles,
 * s >= 0:  phi(t; c, s, kappa) = exp(-s (t - c)^2) (cos(kappa t) - i sin(kappa t));  s = 0 is a plane wave (the Gaussian
 * part is then exactly 1), a beam of 1/e field radius w has s = 1 / w^2.  With la x-factors and lb y-factors,
 *   out_host[c][m][b][a] = sum over the elements e and the 16 points q of the degree-8 rule of
 *                          |det J_e| w_q u_(c,m)(x_eq) phi(X_eq; xfac_a) phi(Y_eq; yfac_b)      (re, im),
 * every component c < ncomp on its own; (X, Y) the physical quadrature point as the assembly forms it, u the P2 field
 * of the element's six staged rows (a boundary DOF of an indexed record contributes 0), the phase argument the single
 * rounded product kappa t, sincos and exp the full-precision double functions.  Defined on the discrete fields alone:
 * nothing is assumed about the pencil the modes came from.  The reference has no counterpart (it turns no mode vector
 * back into a field).
 * modes_dev: staged by plfem_stage_modes ([ncomp][nrows][k]); indexed as in plfem_sample_fields.  xfac_host [la][3],
 * yfac_host [lb][3] = (c, s, kappa) per factor; they travel to the device inside the work buffer.  Partial tiles per
 * workgroup and a fixed-order second stage: the same bits on every run.  Runs on the locator's stream and
 * synchronises it.
 * work_dev: device scratch of plfem_project_work_bytes(ncomp, k, la, lb) bytes, 256-byte aligned: the result (16 ncomp k
 * la lb bytes), the partial 16 x 16 tiles of every mode -- tiles of 8 x 8 factors, min(256, 1024 / tiles) element slices
 * per tile, at least one, so at most 2 KB ncomp k max(1024, tiles) bytes -- and the two factor tables.
 * Argument errors (ncomp not 1 or 2, k outside [1, 64], la or lb outside [1, 4096], a non-finite factor entry or
 * s < 0, a null pointer, work_bytes too small) return PLFEM_EINVAL with the locator's last error set. */
int plfem_project_work_bytes(int32_t ncomp, int32_t k, int32_t la, int32_t lb, int64_t* bytes);
int plfem_mode_project(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                       int32_t la, const double* xfac_host /* [la][3] = c, s, kappa */,
                       int32_t lb, const double* yfac_host /* [lb][3] */,
                       void* work_dev, int64_t work_bytes, double* out_host /* [ncomp][k][lb][la][2] re, im */);

/* Projection of k staged modes on a batch of sampled complex fields ("frames": an aberrated PSF, a speckle pattern, a
 * measured near field, the output of a beam-propagation run): what each mode receives from each input field.  Frame f
 * holds complex samples on the node grid x_i = x0 + i dx (i < nx), y_j = y0 + j dy (j < ny), dx, dy > 0, and
 *   out_host[c][m][f] = sum over the elements e and the 16 points q of the degree-8 rule of
 *                       |det J_e| w_q u_(c,m)(x_eq) F_f(x_eq)                                  (re, im, no conjugation),
 * every component c < ncomp on its own; (X, Y) = x_eq the physical quadrature point as the assembly forms it, u the P2
 * field of the element's six staged rows (a boundary DOF of an indexed record contributes 0), both exactly as in
 * plfem_mode_project.  F_f is the bilinear interpolant of frame f:
 *   tx = (X - x0) * (1 / dx), 1 / dx formed once on the host, the difference and the product each rounded on their own
 *   (no fused multiply-add); ty likewise.  A point with tx < 0, tx > nx - 1, ty < 0 or ty > ny - 1 contributes 0 (the
 *   extent is closed).  Otherwise i0 = min(floor(tx), nx - 2), a = tx - i0, j0 and b likewise, and
 *   F = ((1 - a) F[j0][i0] + a F[j0][i0+1]) (1 - b) + ((1 - a) F[j0+1][i0] + a F[j0+1][i0+1]) b    for re and im each,
 *   every product rounded on its own; the point's term is (|det J_e| w_q) F.
 * The interpolant is continuous, so the cell a point on a pixel edge falls in does not matter beyond rounding; only the
 * outer edge is a discontinuity.  Frame values are the caller's: a NaN pixel gives NaN results for its frame only.
 * Defined on the discrete fields alone; the reference has no counterpart.
 * modes_dev: staged by plfem_stage_modes ([ncomp][nrows][k]); indexed as in plfem_sample_fields.  frames_dev: device,
 * pixel-major and frame-minor, [ny][nx][nf][2] (re, im): the columns of a workgroup's tile at one pixel corner are one
 * contiguous run; offsets into it are 64-bit (ny nx nf 2 may pass 2^31).  Partial tiles per workgroup and a fixed-order
 * second stage whose slice count depends on the mesh alone: the same bits on every run, and the bits of a frame do not
 * depend on the frames it is batched with.  Runs on the locator's stream and synchronises it.
 * Limits: ncomp 1 or 2, 1 <= k <= 64, 2 <= nx, ny <= 8192, 1 <= nf <= 4096; x0, y0, dx, dy, 1 / dx, 1 / dy finite.
 * work_dev: device scratch of plfem_project_sampled_work_bytes(ncomp, k, nf) bytes, 256-byte aligned: the result (16 ncomp k
 * nf bytes) plus the partial tiles of one launch -- tiles of 32 frames (512 ncomp k bytes each), at most 16 tiles per
 * launch, 128 element slices per tile -- so at most 1 MiB ncomp k more (128 MiB at ncomp k = 128, 44 MiB for 22
 * vectorial modes).
 * Argument errors (ncomp not 1 or 2, k outside [1, 64], nx or ny outside [2, 8192], nf outside [1, 4096], dx or dy not
 * positive or any of x0, y0, dx, dy, 1 / dx, 1 / dy not finite, a null pointer, work_bytes too small, an indexed record
 * on an analysis without interior DOFs) return PLFEM_EINVAL with the locator's last error set, starting
 * "plfem_mode_project_sampled: "; they write nothing and leave the locator usable. */
int plfem_project_sampled_work_bytes(int32_t ncomp, int32_t k, int32_t nf, int64_t* bytes);
int plfem_mode_project_sampled(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                               int32_t nx, int32_t ny, double x0, double y0, double dx, double dy,
                               int32_t nf, const double* frames_dev /* [ny][nx][nf][2] re, im */,
                               void* work_dev, int64_t work_bytes, double* out_host /* [ncomp][k][nf][2] */);

/* A-posteriori error indicators of k staged modes: where the mesh limits the eigenvalues a solve returned.  For mode m
 * with pencil eigenvalue lambda_host[m] (vectorial: beta^2; scalar: -beta^2), element T and its three edges e,
 *   out_host[m][T] = |det J_T| sum_q |det J_T| w_q |r(x_q)|^2 + sum_e c_e |e| int_e |[F . n]|^2 ds,
 * the first sum over the assembly's six-point rule, the edge integral by the two-point Gauss rule s = 1/2 -+ 1/(2 sqrt 3)
 * (exact: the jump of the flux of a P2 field is linear along an edge).  c_e = 1/2 on an interior edge; on an edge of the
 * outer boundary 1 for the scalar pencil (natural boundary: the flux itself is the residual) and 0 for the vectorial one
 * (Dirichlet).  Edges run from the lower to the higher vertex id and the edge point is x_lo + fl(s (x_hi - x_lo)): both
 * neighbours form it identically and see the same permittivity.
 *   ncomp = 1, (K - k0^2 M_eps) u = lambda M u:  F = grad u,  r = -lap u - (k0^2 eps + lambda) u;
 *   ncomp = 2, A = K + alpha_p D - k0^2 M, B = M_(1/eps) with the forms as listed for plfem_mode_grams, w = 1 / eps:
 *     F_x = (-w dy hy + alpha_p dx hx,  w dy hx + alpha_p dx hy),  F_y = (w dx hy + alpha_p dy hx,  -w dx hx + alpha_p dy hy),
 *     r_x = -div F_x - (k0^2 + lambda w) hx,  r_y = -div F_y - (k0^2 + lambda w) hy,
 *     div F taken with w frozen at the point (the second derivatives of a P2 field are constant per element).
 *   Summed against a basis function, int r phi_i over the elements plus the outward fluxes int F . n phi_i over all their
 *   edges reproduce ((A - lambda B) h)_i of the unrestricted matrices: the indicator is the residual of the assembled
 *   pencil, localised.
 * Permittivity: nlayer > 0: the index profile (layers_host, nlayer, eps_bg as for plfem_set_index_profile) and the cores
 * arguments are not read; nlayer = 0: eps_core inside the closed discs of cores_host (ncore in [0, 64], the core test of
 * plfem_assemble_hfield) and eps_clad outside.  Either way a point is decided by the helpers the assembly uses.
 * modes_dev: staged by plfem_stage_modes ([ncomp][nrows][k]); indexed as in plfem_sample_fields (a boundary DOF of an
 * indexed record contributes 0).  The element neighbours ("elem_nbr" [3][ne] i32 of plfem_symbolic_get: the element across
 * local edge (0,1), (1,2), (0,2), -1 on the outer boundary; built on the host on first request) and the eigenvalues travel
 * to the device inside the work buffer.  A workgroup owns 16 consecutive elements and stages their geometry and that of
 * their neighbours once; one lane then forms one (element, mode) value in a fixed operation order, nothing is summed
 * across lanes: the bits of out_host[m][T] depend on mode m, its eigenvalue, the mesh and the material table only -- not on
 * k, on the other modes, on what the work buffer held or on the run.  Runs on the locator's stream and synchronises it.
 * work_dev: device scratch of plfem_indicator_work_bytes(loc, ncomp, k) bytes, 256-byte aligned: k ne doubles, 3 ne int32
 * and k doubles, each part rounded up to 256 bytes.
 * Argument errors (ncomp not 1 or 2, k < 1, a null pointer, a non-finite eigenvalue, k0 or alpha_p, a table
 * plfem_set_index_profile rejects, with nlayer = 0 ncore outside [0, 64] or eps_core / eps_clad not finite and positive,
 * work_bytes too small, an indexed record on an analysis without interior DOFs) return PLFEM_EINVAL with the locator's
 * last error set, before any launch. */
int plfem_indicator_work_bytes(const plfem_locator* loc, int32_t ncomp, int32_t k, int64_t* bytes);
int plfem_mode_indicators(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                          const double* lambda_host /* [k] */, double k0, double alpha_p,
                          const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                          const double* layers_host, int32_t nlayer, double eps_bg,
                          void* work_dev, int64_t work_bytes, double* out_host /* [k][ne] */);

/* Electric field, axial Poynting flux and power Grams of k staged vectorial modes (ncomp = 2 only).  Convention of
 * plfem_sample_fields: fields vary as exp(j (w t - beta z)), H = (hx, hy, j hz_im).  From curl H = j w eps0 eps E, with
 * e = E / Z0 (e has the units of H; Z0 = 376.730313668 ohm) and w = 1 / eps(x):
 *   gx = -(hx,xx + hy,xy),  gy = -(hx,xy + hy,yy)        (-grad of div_t H: constant per element for P2)
 *   Ex = w (beta hy + gy / beta) / k0,  Ey = -w (beta hx + gx / beta) / k0,  Ez_im = -w (dx hy - dy hx) / k0  (Ez = j Ez_im),
 *   Sz = (Ex hy - Ey hx) / 2,
 * hence for two modes m, n of one mesh
 *   P[m][n] = 1/2 int (Ex_m hy_n - Ey_m hx_n) dA = (beta_m M_w[m][n] + G_w[m][n] / beta_m) / (2 k0),
 *   M_w[m][n] = int w (hx_m hx_n + hy_m hy_n)  (symmetric: the M_w of plfem_profile_grams),
 *   G_w[m][n] = int w (gx_m hx_n + gy_m hy_n)  (not symmetric),
 * so the device sums are free of beta and k0.  These are the formulas for any staged P2 field with a given beta, eigenpair
 * or not; the transverse E rests on element-wise second derivatives of a P2 field and converges at first order in h.
 * Material: use_profile != 0: the index profile (layers_host, nlayer in [0, 64], eps_bg as for plfem_set_index_profile) over
 * the locator's sampled map if one is set (plfem_locator_set_index_map); eps_core and eps_clad are not read.
 * use_profile == 0: eps_core in the closed discs of cores_host (ncore in [0, 64], the core test of plfem_assemble_hfield)
 * and eps_clad outside; a map set on the locator is then an argument error.  Either way a point is decided by the helpers
 * the assembly uses.  modes_dev: staged by plfem_stage_modes ([2][nrows][k]); indexed as in plfem_sample_fields (a boundary
 * DOF of an indexed record contributes 0).
 *
 * plfem_flux_grams: out_host[0..3][k][k] = M_w_core, M_w_rest, G_w_core, G_w_rest, every sum over the mesh's own six-point
 * rule with |det J| w_q, split by the closed discs of cores_host whatever the material (ncore = 0: everything is "rest").
 * Grid, tiling and second stage of plfem_mode_grams: the same bits on every run, for a subset or a permutation of the
 * modes, and whatever the work buffer held before.  Synchronises the locator's stream.
 * work_dev: device scratch of plfem_flux_gram_work_bytes(k) bytes, 256-byte aligned: the layout of plfem_profile_grams
 * with nout = 4: nout k^2 doubles, rounded up to 256 bytes, plus nout ceil(k / 32)^2 x 768 partial blocks of 8 KiB.
 *
 * plfem_sample_efields: one lane per point (points_dev [2][npts], located as in plfem_sample_fields: same containment and
 * tie rule), eps taken at the point itself; out_dev[0..3][k][npts] = Ex, Ey, Ez_im, Sz; eps_dev[npts] (or NULL) the
 * permittivity used; elem_dev[npts] the element, -1 for a point in no element, whose outputs and eps are 0.  beta_dev [k]
 * is device memory and is not validated: the kernel writes what the arithmetic gives (beta = 0: inf / NaN).  Runs on the
 * locator's stream and synchronises it.  npts = 0 returns PLFEM_OK without a launch.
 *
 * Argument errors return PLFEM_EINVAL with the locator's last error set, before any launch, checked in this order:
 * ncomp != 2 or k < 1 (plfem_sample_efields: or npts < 0); ncore outside [0, 64]; a null array (eps_dev may be NULL);
 * use_profile != 0: a table plfem_set_index_profile rejects, eps_bg included; use_profile == 0: eps_core or eps_clad not
 * finite and positive, then a map set on the locator; plfem_sample_efields: k0 not finite and positive; an indexed record
 * on an analysis without interior DOFs; plfem_flux_grams: work_bytes too small, then a misaligned buffer.
 * plfem_flux_gram_work_bytes rejects k < 1 and a null bytes (left alone). */
int plfem_flux_gram_work_bytes(int32_t k, int64_t* bytes);
int plfem_flux_grams(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                     const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                     const double* layers_host, int32_t nlayer, double eps_bg, int32_t use_profile,
                     void* work_dev, int64_t work_bytes, double* out_host /* [4][k][k] */);
int plfem_sample_efields(plfem_locator* loc, int32_t ncomp, int32_t k, const double* modes_dev, int32_t indexed,
                         const double* beta_dev /* [k] */, double k0,
                         const double* cores_host, int32_t ncore, double eps_core, double eps_clad,
                         const double* layers_host, int32_t nlayer, double eps_bg, int32_t use_profile,
                         int32_t npts, const double* points_dev, double* out_dev /* [4][k][npts] */,
                         double* eps_dev /* [npts] or NULL */, int32_t* elem_dev);
/* Posed flux overlap: the cross flux int (E_a x H_b + E_b x H_a) . z of two vectorial mode sets on two meshes under nposes
 * poses of mesh A relative to mesh B, as four matrices per pose that are free of beta, k0 and m.  Vectorial records only
 * (both mode sets staged [2][nrows][k]).  The pose contract of plfem_field_overlap_posed applies unchanged: a pose row is
 * (tx, ty, c, s, m), B's quadrature point (X, Y) is looked up in A at
 *   xa = (fl(c dx) + fl(s dy)) / m,  ya = (fl(c dy) - fl(s dx)) / m,  dx = X - tx, dy = Y - ty
 * (the identity pose gives (X, Y) bit for bit; the location decisions are those of plfem_sample_fields).  With
 *   hA' = R hA(xa, ya),  gA' = R gA,  g = (-(hx,xx + hy,xy), -(hx,xy + hy,yy)) from the physical Hessians of the element
 *   (as plfem_flux_grams forms it; no factor of m: the host owns every m, beta and k0),
 *   hB, gB: B's own at its quadrature point,  wA = 1 / eps_A at (xa, ya) in A's frame,  wB = 1 / eps_B at (X, Y),
 * out_host[p][0..3][ka][kb] = MA, GA, MB, GB, every sum over the elements of B and B's six-point rule with |det J| w_q:
 *   MA[i][j] = sum wA (hA'_i . hB_j)      GA[i][j] = sum wA (gA'_i . hB_j)
 *   MB[i][j] = sum wB (hA'_i . hB_j)      GB[i][j] = sum wB (hA'_i . gB_j).
 * A point that lands in no element of A contributes 0 to all four; a boundary DOF of an indexed record contributes 0.
 * With X_ab = (beta_a MA + GA / beta_a) / k0_a = int (E_a' x H_b) . z and X_ba = (beta_b MB + GB / beta_b) / k0_b =
 * int (E_b x H_a') . z (beta_a along the rows, beta_b along the columns; k0_b = k0_a / m: the magnified field has every
 * wavenumber divided by m and g by m^2, so its E is A's own E turned and its power m^2 P_a) the power-normalised
 * transfer is (X_ab + X_ba)[i][j] / (4 m sqrt(|P_a,i| |P_b,j|)).
 * Material of each side, a flat argument set as in plfem_flux_grams: use_profile == 0: eps_core in the closed discs of
 * cores (ncore in [0, 64]) and eps_clad outside; use_profile != 0: the layer profile (layers, nlayer, eps_bg).  Either way
 * a point is decided by the helpers the assembly uses.  Each side's layer table travels through its own locator's device
 * buffer; with one locator on both sides and a profile on both, the two tables must be the same.  Sampled index maps are
 * out of scope of this call: a map set on either locator is an argument error, whatever use_profile says.
 * One workgroup per (slice of B's 32-point tiles, pair of 32-mode chunks, pose) writes its four partial blocks to their own
 * slots, slices = min(128, tiles of B) whatever nposes, ka and kb are, and the fixed-order second stage of
 * plfem_field_overlap sums them: no atomics, and the bits of out_host[p] depend on pose p, the modes, the materials and the
 * two meshes only -- not on the other poses, on nposes, on the batch boundary, on what the work buffer held, on the run, or
 * on a permutation of the modes of either side.  The poses are worked off in batches of
 *   batch = max(1, min(nposes, 4096, (512 MiB - 768) / (8 (4 ka kb + 4096 pairs slices + 5)))) poses,
 * pairs = ceil(ka / 32) ceil(kb / 32) <= 64 -- a quarter of plfem_field_overlap_posed's limit, so that one pose of the
 * largest call (256 MiB of partial blocks) still fits -- and work_dev holds one batch: its results [batch][4][ka][kb], its
 * partial blocks [batch][4][pairs][slices][1024] and its pose rows, each part 256-byte aligned, so
 * plfem_flux_overlap_posed_work_bytes(loc_b, ka, kb, nposes) never exceeds 512 MiB.  Runs on loc_a's stream and
 * synchronises it once, at the end; both locators on one device.
 * Argument errors return PLFEM_EINVAL with loc_a's last error set, before any launch, checked in this order: loc_b null
 * or on another device; ka or kb < 1, nposes < 1, more than 64 chunk pairs; ncore of a side outside [0, 64]; a null
 * array (cores only with ncore > 0); side A's material, then side B's, each by the rules of plfem_flux_grams (a profile's
 * table, or the discs' two permittivities) followed by a map set on that side's locator; one locator on both sides with
 * two different layer tables; an indexed record on an analysis without interior DOFs; a non-finite pose entry, m <= 0 or
 * |c^2 + s^2 - 1| > 1e-12; work_bytes too small, then a misaligned buffer.  A null loc_a returns PLFEM_EINVAL alone.
 * plfem_flux_overlap_posed_work_bytes rejects a null loc_b or bytes (left alone), ka, kb or nposes < 1 and more than 64
 * chunk pairs. */
int plfem_flux_overlap_posed_work_bytes(const plfem_locator* loc_b, int32_t ka, int32_t kb, int32_t nposes, int64_t* bytes);
int plfem_flux_overlap_posed(plfem_locator* loc_a, const double* modes_a_dev, int32_t ka, int32_t indexed_a,
                             const double* cores_a_host, int32_t ncore_a, double eps_core_a, double eps_clad_a,
                             const double* layers_a_host, int32_t nlayer_a, double eps_bg_a, int32_t use_profile_a,
                             plfem_locator* loc_b, const double* modes_b_dev, int32_t kb, int32_t indexed_b,
                             const double* cores_b_host, int32_t ncore_b, double eps_core_b, double eps_clad_b,
                             const double* layers_b_host, int32_t nlayer_b, double eps_bg_b, int32_t use_profile_b,
                             int32_t nposes, const double* poses_host /* [nposes][5] = tx, ty, c, s, m */,
                             void* work_dev, int64_t work_bytes, double* out_host /* [nposes][4][ka][kb] */);

#ifdef PLFEM_TEST_HOOKS
/* ---------------------------------------------------------------------------------------------
 * TEST HOOKS -- NOT exported by libplfem_hip.so.  They live in the add-on libplfem_testhooks.so (csrc/api_debug.hip,
 * built next to the product library and linked against it), which only tests/ and scripts/ load; define
 * PLFEM_TEST_HOOKS before including this header to see the declarations.  They take contexts created by the product
 * library and run the product library's own kernels.
 * Debugging aids for the test-suite (no reference counterpart): run the factorisation only up to
 * a given (tree level, block step, stage: 0 assembled, 1 or 2 pivot block + panel of the step done (its own launch for
 * step 0 of a level, the launch of the step before otherwise), 3 or 4 the step's launch done: trailing update + inverse
 * row + pivot write-back, next pivot block + panel; 5 level done), and copy a slice of a named device workspace
 * ("front","schur","fvec","fvec2","xl","wbuf","rbuf","dinv","delta","elem"; "colind","slot_row": the device-built CSR
 * index arrays, converted to double).  "schur", "wbuf" and "rbuf" -- scratch of the factorisation -- share their part of the
 * workspace with the Lanczos bases: copy them before the next plfem_lanczos_shift_invert / plfem_solve of the context.
 * plfem_debug_symeig: the host eigensolver of the Lanczos drivers (projected matrices of order
 * <= ~200; needs no GPU).  a_host: n x n symmetric.  last_rows < 0: v_out[i*n + k] = component k of
 * eigenvector i; last_rows = p >= 0: v_out[i*p + a] = component n-p+a of eigenvector i only (the
 * cheap form used by the per-step convergence test).  w_out[n]: eigenvalues, same (arbitrary) order.
 * plfem_debug_symeig_band: the band path used for the final Ritz vectors of a run without restart
 * (half bandwidth b; entries further from the diagonal are ignored): w_out[n] ascending, v_out[i*n + k] =
 * component k of the eigenvector of w_out[i] for the nsel eigenvalues of largest magnitude, zero rows elsewhere.
 * ------------------------------------------------------------------------------------------- */
int plfem_debug_factor_until(plfem_ctx* ctx, double sigma, int32_t level, int32_t step, int32_t stage);
int plfem_debug_copy(plfem_ctx* ctx, const char* name, int64_t offset, int64_t count, double* out_host);
int plfem_debug_symeig(int32_t n, const double* a_host, int32_t last_rows, double* w_out, double* v_out);
int plfem_debug_symeig_band(int32_t n, int32_t b, const double* a_host, int32_t nsel, double* w_out, double* v_out);
/* fault injection for the a-posteriori guard: from the next plfem_factor on, D^-1 of the root front is scaled by
 * 1 + value after every factorisation (0 = off) */
int plfem_debug_set_perturb(plfem_ctx* ctx, double value);
/* the write counterpart of plfem_debug_copy("elem"): elem_host replaces the element matrices of the context (every slot
 * of every element, [i][j] row-major), the product's CSR gather rebuilds the assembled blocks from them, and the context
 * is assembled and not factored: plfem_factor, plfem_spmv and the refinement inside the solves all see this pencil.
 * Synchronises. */
int plfem_debug_set_elements(plfem_ctx* ctx, const double* elem_host /* [ne][PLFEM_BLK_COUNT][36] */);
/* plfem_debug_solve_block: BLOCK_P (4) right-hand sides in global order, column u at rhs_dev + u ldx, through the block
 * sweeps the block Lanczos driver runs (k_permute_in / k_permute_out and the P = 4 sweep kernels); the solutions go to
 * the same columns of x_dev.  refine_steps passes of block iterative refinement against the assembled K = A - sigma B
 * follow (block SpMVs; scratch: the Lanczos restart buffer, so 3 BLOCK_P ldx <= n2 (max_ncv + 1 + BLOCK_P)).  Nothing
 * outside the n2 entries of each column is read or written.  PLFEM_ESTATE before plfem_factor; PLFEM_EINVAL when the
 * LDS budget of the tree rules out P = 4 sweeps (largest front too large), when ldx < n2 or the scratch is too small.
 * Synchronises.
 * plfem_debug_level_plan: the context's launch plan, PLFEM_DEBUG_PLAN_FIELDS int64 per tree level (level 0 = root,
 * cap >= that times L + 1): fronts, forward rows per workgroup (8 / 16: row form, 64: tile form), backward rows per
 * workgroup (64: the leaf level's tile form), 1 if the forward launch is mixed (tiles + row jobs), largest s2, largest m,
 * forward workgroups, backward workgroups, block steps of the factorisation, right-hand sides per sweep allowed. */
#define PLFEM_DEBUG_PLAN_FIELDS 10
int plfem_debug_solve_block(plfem_ctx* ctx, const double* rhs_dev, int64_t ldx, double* x_dev, int32_t refine_steps);
int plfem_debug_level_plan(plfem_ctx* ctx, int64_t* out, int64_t cap);
/* The device kernels of the two Lanczos drivers on caller device buffers, for the kernel-level tests (each hook runs the
 * product's own launch function on the context's stream and synchronises).  Vectors have n2 = dofs_per_node N entries
 * (component-major); column c of a panel Pm starts at Pm + c n2, column q of a block at W + q ldw (ldw >= n2).
 * plfem_debug_panel, 1 <= ncols <= max_ncv + BLOCK_P:
 *   PLFEM_DEBUG_PANEL_DOT        H[c] = Pm[:, c] . W (single-vector driver, the P = 1 instance of the block form; W one
 *                                vector); hacc (may be NULL): hacc[c] += the same
 *   PLFEM_DEBUG_PANEL_AXPY       W -= Pm H[0:ncols]
 *   PLFEM_DEBUG_PANEL_DOT_BLOCK  H[c + q ldh] = Pm[:, c] . W[:, q], q < BLOCK_P; hacc (may be NULL): hacc[c + q ldacc] += the same
 *   PLFEM_DEBUG_PANEL_AXPY_BLOCK W[:, q] -= sum_c Pm[:, c] H[c + q ldh]; wil (may be NULL, n2 BLOCK_P): the updated block
 *                                interleaved, wil[(node dofs_per_node + component) BLOCK_P + q]
 * plfem_debug_scale_store: v = w / beta, bv = bw / beta, beta = sqrt(max(*beta2, 0)) (zero vectors when beta = 0), beta ->
 *   *beta_out (device, may be NULL); beta2 is a device pointer.
 * plfem_debug_first_pass: xl_front (2 fnode_ptr[nfronts] BLOCK_P doubles, the sweeps' front-order result) is copied into the
 *   context's backward-sweep buffer, then the fused first Gram-Schmidt pass of a block step: W = the block in global order
 *   (Dirichlet rows 0), h = BVm^T W -> Hout[c + q ldh], W -= Vm h; 1 <= ncols <= 8.
 * plfem_debug_spmv_block (after assembly): y[:, q] = B x[:, q] (PLFEM_DEBUG_SPMV_B_BLOCK), the same with x interleaved as wil
 *   above (..._IL), and with the Gram partials of x^T (B x) (..._IL_GRAM: *nparts partials per entry, gram_out[(p BLOCK_P + q)
 *   nparts + b] when gram_out is not NULL; they also stay where plfem_debug_chol with use_partials and G = NULL reads them),
 *   y[:, q] = A x[:, q] (PLFEM_DEBUG_SPMV_A_BLOCK); columns ld apart.
 * plfem_debug_chol: G = R^T R of a BLOCK_P x BLOCK_P matrix, ready-made (G[i + j ldg], use_partials = 0) or as nchunks partials
 *   per entry (use_partials = 1; G = NULL: the partials the last ..._IL_GRAM product left).  R -> Tblk[i + j ldT], R^-1 ->
 *   Rinv[i + j BLOCK_P] (device); *rank_flag = non-positive pivots met (each replaced by 1).
 * plfem_debug_block_scale: Vn = W R^-1, BVn = BW R^-1 (Rinv as above; columns ldv apart); exp_dst (may be NULL): exp_dst[0:exp_n]
 *   = exp_src[0:exp_n] and cnt_dst[0:4] = the device counters (plfem_debug_copy "counters"); want_front: BVn also to the
 *   front-order buffer "fvec" (BLOCK_P values per DOF together).
 * plfem_debug_rotate: out[:, 0:p] = V[:, 0:m] S[0:m, 0:p] (S[r + c ldS]; columns n2 apart), 1 <= m <= PLFEM_MAX_NCV + BLOCK_P.
 * plfem_debug_start_field: the start block of the drivers, nvec <= BLOCK_P vectors (n2 apart) of the 64-bit LCG stream over
 *   (vector, component, interior DOF), Dirichlet entries 0.
 * plfem_debug_copy also knows "V", "BV" (the Lanczos basis and B times it, n2 per column) and "Hcols" (the device projected
 * matrix, column major with leading dimension ld = m + P for a basis of m columns and blocks of P vectors: P = BLOCK_P for
 * the block driver, 1 for the single-vector one), valid after a run without restart (a restart swaps the bases), and
 * "counters" (the 4 int32 device counters, [2] the rank flag of the block driver). */
enum { PLFEM_DEBUG_PANEL_DOT = 0, PLFEM_DEBUG_PANEL_AXPY, PLFEM_DEBUG_PANEL_DOT_BLOCK, PLFEM_DEBUG_PANEL_AXPY_BLOCK };
enum { PLFEM_DEBUG_SPMV_B_BLOCK = 0, PLFEM_DEBUG_SPMV_B_BLOCK_IL, PLFEM_DEBUG_SPMV_B_BLOCK_IL_GRAM, PLFEM_DEBUG_SPMV_A_BLOCK };
int plfem_debug_panel(plfem_ctx* ctx, int32_t form, int32_t ncols, const double* Pm, double* W, int64_t ldw, double* H,
                      int32_t ldh, double* hacc, int32_t ldacc, double* wil);
int plfem_debug_scale_store(plfem_ctx* ctx, const double* w, const double* bw, const double* beta2, double* v, double* bv,
                            double* beta_out);
int plfem_debug_first_pass(plfem_ctx* ctx, const double* xl_front, const double* BVm, const double* Vm, int32_t ncols,
                           double* W, int64_t ldw, double* Hout, int32_t ldh);
int plfem_debug_spmv_block(plfem_ctx* ctx, int32_t form, const double* x, double* y, int64_t ld, double* gram_out,
                           int32_t* nparts);
int plfem_debug_chol(plfem_ctx* ctx, const double* G, int32_t ldg, int32_t use_partials, int32_t nchunks, double* Tblk,
                     int32_t ldT, double* Rinv, int32_t* rank_flag);
int plfem_debug_block_scale(plfem_ctx* ctx, const double* W, const double* BW, int64_t ldw, const double* Rinv, double* Vn,
                            double* BVn, int64_t ldv, const double* exp_src, int32_t exp_n, double* exp_dst, int32_t* cnt_dst,
                            int32_t want_front);
int plfem_debug_rotate(plfem_ctx* ctx, const double* V, int32_t m, const double* S, int32_t ldS, int32_t p, double* out);
int plfem_debug_start_field(plfem_ctx* ctx, int32_t nvec, double* out);
#endif /* PLFEM_TEST_HOOKS */

#ifdef __cplusplus
}
#endif
#endif /* PLFEM_H */
