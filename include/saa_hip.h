/*
 * saa_hip.h - C ABI of libsaa_hip.so: the MI355X (gfx950) implementation of the explicit
 * linear-tetrahedral elastodynamics hot path of desResLab/Synchronization-avoiding-algorithms.
 *
 * The reference has no FFI: its hot path sits behind Python call signatures
 * (SURVEY.md section 8(b)).  Each entry point below names the reference interface it replaces
 * (file:line in /root/reference); INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.  Plain pointers and sizes only; no torch / numpy types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative SAA_E_* code otherwise; the message of the
 *     last failure on the calling thread is returned by saa_last_error().
 *   - "host" pointers are caller-owned CPU buffers, "dev" pointers caller-owned device buffers
 *     (e.g. torch tensors' data_ptr()).  The library never frees caller memory.
 *   - node / dof numbering at this boundary is ALWAYS the caller's (the rank-local first-touch
 *     numbering of Distributed_tools.py:14-24; dof = 3*node + component, commons.py:66-71).
 *     Internally nodes are renumbered block-wise; that never shows through the ABI.
 *   - one handle per GPU partition; calls on one handle must be serialised by the caller.  All
 *     device work is enqueued on the stream given to saa_set_stream (default: the null stream),
 *     so PyTorch-ROCm and RCCL work ordered on the same stream needs no extra synchronisation.
 *   - fp64 throughout (the reference is float64 NumPy).
 */
#ifndef SAA_HIP_H
#define SAA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAA_OK 0
#define SAA_E_ARG (-1)     /* bad argument (null pointer, index out of range, degenerate element) */
#define SAA_E_HIP (-2)     /* a HIP runtime call failed (no device, out of memory, launch failure) */
#define SAA_E_STATE (-3)   /* call sequence error (e.g. step_finish without step_begin) */
#define SAA_E_CAPACITY (-4) /* a node block does not fit the LDS budget even at the smallest size */

typedef struct saa_solver saa_solver;

/*
 * Everything one rank holds after the set-up of Data_prepare.py:104-209, in the caller's numbering.
 */
typedef struct saa_problem {
  int32_t n_nodes;               /* len(Local_nodal_list), Data_prepare.py:104 */
  int32_t n_elems;               /* len(Local_ele_list) */
  const double *xyz;             /* host (n_nodes,3): Points[Local_nodal_list] */
  const int32_t *tets;           /* host (n_elems,4): local node ids (local_mat_node of Cells rows,
                                    Mat_construction.py:139) */
  const double *lumped_mass;     /* host (3*n_nodes): l_M, Data_prepare.py:202 */
  const double *f_ext;           /* host (3*n_nodes): F_rankwise (un-ramped), Data_prepare.py:201 */
  const int32_t *dirichlet_dofs; /* host (n_dirichlet): Local_Dirichlet, Data_prepare.py:144 */
  int32_t n_dirichlet;
  const int32_t *shared_nodes;   /* host (n_shared): local ids of this rank's shared nodes, in the
                                    order of `shared_nodes` (Data_prepare.py:112); defines the column
                                    order 3*i+c of the LSTM input (Online_predictor.py:126-129) */
  const int32_t *shared_slots;   /* host (n_shared): position of each shared node in the sorted
                                    Global_shared list (Data_prepare.py:121-124) */
  int32_t n_shared;
  int32_t n_global_shared;       /* len(Global_shared); interface buffer holds 3*n_global_shared */
  double lambda_;                /* elasticity.lmd, commons.py:17 */
  double mu;                     /* elasticity.mu */
  double dt;                     /* min CFL step, Data_prepare.py:147-154 */
  double alpha;                  /* mass-proportional damping `Damp`, Data_prepare.py:41 */
  int32_t ramp;                  /* 1: F_ext = F_rankwise*min(t,1) (Dynamic_solver.py:13); 0: constant */
  int32_t device;                /* HIP device ordinal */
  int32_t block_nodes;           /* target owned nodes per workgroup; 0 = automatic */
  int32_t threads;               /* workgroup size (multiple of 64, <= 1024); 0 = automatic */
} saa_problem;

/* Statistics of the block decomposition (for DESIGN.md / bench.py roofline bookkeeping). */
typedef struct saa_plan_stats {
  int32_t n_blocks;
  int32_t max_owned;        /* owned nodes of the largest block */
  int32_t max_local;        /* owned + halo nodes of the largest block */
  int64_t n_elem_copies;    /* sum over blocks of elements touching the block (>= n_elems) */
  int64_t n_halo_total;     /* sum over blocks of halo nodes */
  int32_t lds_bytes;        /* dynamic LDS per workgroup */
  int32_t threads;          /* workgroup size in use */
  double lds_conflict_factor; /* mean worst LDS bank multiplicity of the record reads per (lane group, vertex slot); 1 = none */
  double lds_atomic_conflict_factor; /* the same for the force accumulation (ds_add_f64) per (half-wave, vertex slot) */
  int64_t n_items;          /* work items (pairs of face-adjacent elements, single elements, idle slots of the packing) */
  int64_t n_pairs;          /* items that hold two elements */
  int64_t n_by_construction; /* item slots in half-waves that are clash-free by construction (pattern classes) */
  int32_t n_renumbered;     /* blocks whose nodes took another order than the plan's first choice (axis order / pseudo-lattice) */
  int32_t reserved;
} saa_plan_stats;

const char *saa_last_error(void);
/* Library / ABI version; bumps when this header changes (2: peer exchange and resident-kernel entry points; 3: loop-back attach; 4: partitioner and set-up kernels; 5: deterministic mode; 6: copy-bandwidth aid; 7: saa_plan_stats grew; 8: saa_predictor_*, saa_topology_*; 9: saa_set_option, saa_plan_stats.n_renumbered; 10: saa_plan_host_check; 11: saa_operator_*; 12: saa_operator_stress, saa_operator_nodal_average; 13: saa_plan_host_block_maxima; 14: saa_operator_stress_error; 15: saa_operator_create_p2, saa_operator_order, saa_operator_load, saa_operator_diagonal; 16: saa_operator_lumped_mass, saa_operator_stepper_*; the p = 2 stress entry points saa_operator_stress_p2, saa_operator_nodal_stress_p2 and saa_operator_stress_error_p2 joined version 16 without a bump: they add symbols and change no declaration; so did the partition entry points of the operator stepper, saa_operator_stepper_set_shared, _set_interface_buffer, _step_begin, _step_finish, _step_predicted, _halo_gather and _halo_scatter, then saa_operator_stepper_set_energy, the finite-strain entry points and saa_operator_tangent_apply, then saa_operator_shifted_apply and saa_operator_implicit_*). */
int32_t saa_abi_version(void);

/* Element partition, one part per rank / GPU: the role of `_, epart = part_mesh_kway(size, eptr, eind)` (mgmetis /
 * ParMETIS, Data_prepare.py:82-101).  Graph partitioning of the dual graph (elements adjacent across a face): recursive
 * bisection by greedy graph growing + Fiduccia-Mattheyses refinement; deterministic, host only, no HIP call - every rank
 * computes the same vector from the replicated mesh (Data_prepare.py:76-79) instead of running a distributed partitioner.
 * tets: (n_elems,4) node ids in [0, n_nodes); epart_out: (n_elems) part of every element; stats_out may be NULL. */
typedef struct saa_partition_stats {
  int64_t face_cut;          /* faces between elements of different parts */
  int64_t min_part, max_part; /* elements in the smallest / largest part */
  int32_t interface_nodes;   /* nodes touched by more than one part = len(Global_shared), Data_prepare.py:121-124 */
} saa_partition_stats;
int saa_part_mesh_kway(int32_t n_parts, int32_t n_elems, int32_t n_nodes, const int32_t *tets, int32_t *epart_out,
                       saa_partition_stats *stats_out);

/* Set-up fields on the GPU, O(N), for the elements given (a rank passes the elements touching its own nodes):
 *   lumped_mass_out (3*n_nodes): row sums of the consistent mass = sum_e rho*V_e/4 per node, on its three dofs
 *                                (Global_Assembly_no_bc + lumping_to_vec: Mat_construction.py:199-231, commons.py:103-107,
 *                                Data_prepare.py:175-176);
 *   f_pre_out       (3*n_nodes): pre-assembled un-ramped body force sum_e (V_e/4)*(0,-fz,-fz) (same call, F_pre);
 *   min_edge_out    (scalar)   : shortest element edge; Meshsize = 2*min_edge/sqrt(24) (commons.py:79-90), from which
 *                                dt = gamma*Meshsize/sqrt(E/rho/(1-nu^2)) (Data_prepare.py:147).
 * Replaces the reference's dense (3N)^2 assembly on rank 0.  Signed volumes (detJ/6, Mat_construction.py:93); no
 * floating-point atomics: nodal sums run in ascending element order (deterministic).  Host pointers in and out, any
 * output may be NULL. */
int saa_setup_fields(int32_t device, int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets, double rho,
                     double fz, double *lumped_mass_out, double *f_pre_out, double *min_edge_out);

/* Build the device-resident solver for one partition.  Replaces, for this path,
 * Local_assembly_for_stiffness (Mat_construction.py:122-150: no matrix is ever assembled) plus the
 * per-step argument marshalling of parallel_explicit_solver_dis_pre (Dynamic_solver.py:9-10).
 * Initial state is d0 = dn = 0, tn = 0 (Data_prepare.py:171-172,215). */
int saa_create(const saa_problem *problem, saa_solver **out);
int saa_destroy(saa_solver *s);
int saa_plan_stats_get(const saa_solver *s, saa_plan_stats *out);

/* Host-only plan builder (no HIP call): same decomposition saa_create uses, for CPU tests. */
int saa_plan_host_stats(int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets,
                        int32_t block_nodes, saa_plan_stats *out);
/* Self-check of the block plan the library would build for this partition (host only, no GPU): the internal numbering is a
 * permutation; every work item names valid nodes, its tets are elements of the mesh in the mesh's orientation (the signed
 * detJ of Mat_construction.py:93), first-round items name owned nodes only; every element appears exactly once in every
 * block owning one of its nodes and nowhere else.  *violations_out = number of failed checks (0: the plan is what the step
 * kernels assume).  No reference counterpart (its LocalK is an assembled matrix); used by the CPU tests. */
int saa_plan_host_check(int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets, int32_t block_nodes,
                        int64_t *violations_out);
/* Per-block extremes of that plan (host only, no GPU; saa_plan_stats holds maxima of the node counts and totals only):
 * out6 = { largest halo, largest work-item list, largest interior list, largest boundary list (items - interior),
 * smallest owned count, smallest halo } over the blocks.  The CPU tests prove with them which sweep-depth regime of the
 * step kernels a (mesh, block_nodes, threads) point reaches. */
int saa_plan_host_block_maxima(int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets, int32_t block_nodes,
                               int32_t *out6);

/* All later work of this handle goes to `hip_stream` (a hipStream_t; NULL = null stream). */
int saa_set_stream(saa_solver *s, void *hip_stream);

/* Time_integration_displacement(tn, dt, d0, dn) (commons.py:47-55): d0 = d^n, dn = d^(n-1). */
int saa_set_state(saa_solver *s, const double *d0_host, const double *dn_host, double tn);
int saa_get_state(saa_solver *s, double *d0_host, double *dn_host, double *tn);
/* Same, into caller-owned DEVICE buffers of 3*n_nodes doubles (either may be NULL). */
int saa_get_state_device(saa_solver *s, double *d0_dev, double *dn_dev);
/* Replace the un-ramped external force / lumped mass (host, 3*n_nodes each; NULL = keep). */
int saa_set_loads(saa_solver *s, const double *f_ext_host, const double *lumped_mass_host);

/* f = K_local . d without K: backs `LocalK.dot(T.d0)` (Dynamic_solver.py:12).  Host in, host out,
 * 3*n_nodes doubles each. */
int saa_internal_force(saa_solver *s, const double *d_host, double *f_host);
/* Same with caller-owned DEVICE buffers (3*n_nodes doubles each, caller numbering), enqueued on the handle's stream:
 * the operator of iterative solvers that keep their vectors on the GPU - the matrix-free replacement of
 * `np.linalg.solve(K, F)` in Steady_Elasticity_solver (Tools/Steady_solvers.py:13-22, Data_prepare.py:163). */
int saa_internal_force_device(saa_solver *s, const double *d_dev, double *f_dev);

/* One damped central-difference update on the host-provided arrays, evaluated on the GPU in the
 * reference's association order (Dynamic_solver.py:13-20).  Backs the drop-in
 * parallel_explicit_solver_dis_pre when the caller owns the state. */
int saa_cd_update(saa_solver *s, const double *f_int_host, const double *d0_host, const double *dn_host,
                  double tn, double *d1_host);

/* nsteps explicit steps with no exchange: the serial case (size == 1) and the MODEL=True branch
 * of Dynamic_solver.py:22 without a halo overwrite.  State rotates (dn<-d0<-d1), tn += dt. */
int saa_step(saa_solver *s, int32_t nsteps);

/* Synchronised step, split around the caller's collective (replaces syn_cpus,
 * Distributed_tools.py:77-92, by an all-reduce over the compact interface buffer):
 *   saa_step_begin : interior + shared nodes get the local update; the partial K_r d of every
 *                    local shared node is written to iface_dev[3*slot+c]; slots of shared nodes
 *                    this rank does not hold stay 0.
 *   (caller: all-reduce(sum) of iface_dev over ranks, on the same stream)
 *   saa_step_finish: shared nodes are recomputed from the summed force (Dynamic_solver.py:26-32),
 *                    non-local slots are re-zeroed, state rotates, tn += dt.  If hist_dev != NULL the
 *                    new shared-dof values are also written to hist_dev[hist_row*3*n_shared + ...]
 *                    (Online_predictor.py:260). */
int saa_set_interface_buffer(saa_solver *s, double *iface_dev);
int saa_step_begin(saa_solver *s);
int saa_step_finish(saa_solver *s, double *hist_dev, int64_t hist_row);

/* Optional native exchange: the per-step all-reduce issued from C++ on the handle's stream through the
 * RCCL library that is already loaded in the process (e.g. PyTorch-ROCm's librccl.so, given by path), so that
 * a synchronised step costs three enqueues and no interpreter time.
 *   saa_comm_unique_id : rank 0 creates the 128-byte ncclUniqueId; the caller broadcasts it to every rank
 *   saa_comm_init      : every rank joins (ncclCommInitRank); needs saa_set_interface_buffer first
 *   saa_step_synced    : nsteps x (saa_step_begin, ncclAllReduce(sum, fp64) of the interface buffer,
 *                        saa_step_finish); history rows hist_row0 + k as in saa_step_finish
 * With world == 1 the collective is the identity (used by the single-GPU tests). */
int saa_comm_unique_id(const char *rccl_path, uint8_t id_out[128]);
int saa_comm_init(saa_solver *s, const char *rccl_path, const uint8_t id[128], int32_t rank, int32_t world);
int saa_step_synced(saa_solver *s, int32_t nsteps, double *hist_dev, int64_t hist_row0);

/* Direct peer exchange: the synchronised step without a collective and without a second kernel.  Inside the fused
 * step kernel the partial force of every shared node is stored straight into the memory of the other ranks holding
 * that node (fine-grained device memory mapped through HIP IPC; xGMI peer stores; every 16-byte entry carries the
 * step's sequence number, so it is its own "ready" flag) and every rank sums what it received in RANK ORDER - the
 * summation order of syn_cpus (Distributed_tools.py:84-86), so all ranks obtain identical bits.  Only ranks with a
 * common shared node talk to each other; the xGMI flight time hides under the update of the non-shared nodes.
 *   saa_peer_export   : allocates this rank's inbox and returns its 64-byte hipIpcMemHandle_t plus, per shared
 *                       node, its position in this rank's push order (order_out, n_shared values); the caller
 *                       all-gathers handles, device ordinals, shared_slots lists and push orders of every rank
 *                       (any transport: torch.distributed, MPI, files)
 *   saa_peer_attach   : maps the inboxes of the neighbours (ranks with a common slot) and builds the push / receive
 *                       lists; handles = world x 64 bytes, devices[world], slot_counts[world], slots / orders = the
 *                       ranks' lists concatenated in rank order (this rank's slots must equal saa_problem's)
 *   saa_peer_selftest : COLLECTIVE over the attached ranks: one exchange of known values; *ok = 1 iff every
 *                       sum arrived intact within the time limit.  The caller agrees on min(ok) over ranks
 *                       before relying on saa_step_peer, and otherwise keeps the all-reduce path
 *   saa_step_peer     : nsteps synchronised steps, ONE kernel launch each; history rows as in saa_step_finish
 * Waits inside the kernel are bounded (30 s, env SAA_PEER_TIMEOUT_S): a dead neighbour turns into SAA_E_STATE at
 * the next saa_synchronize / saa_get_state instead of a hang. */
int saa_peer_export(saa_solver *s, int32_t world, uint8_t handle_out[64], int32_t *order_out);
int saa_peer_attach(saa_solver *s, int32_t rank, int32_t world, const uint8_t *handles, const int32_t *devices,
                    const int32_t *slot_counts, const int32_t *slots, const int32_t *orders);
int saa_peer_selftest(saa_solver *s, int32_t *ok);
/* Single-GPU rehearsal of the peer exchange (instead of saa_peer_export + saa_peer_attach): this handle becomes rank 0
 * of `world` (2..8) ranks whose other members are imaginary - they hold exactly this rank's shared nodes and their
 * inbox segments live in this rank's own inbox, so every pushed value comes straight back.  saa_step_peer then runs the
 * complete push / stamp / poll / rank-ordered-sum path of a real multi-GPU step with local instead of xGMI latency, and
 * the force a shared node is updated with is exactly world x its local partial force (a + a + ... in rank order) - a
 * well-defined operator the parity tests reproduce on the CPU (tests/test_gpu_fullsize.py: the per-GPU workload of the
 * 8-GPU configuration checked on one GPU).  Needs n_shared > 0. */
int saa_peer_attach_loopback(saa_solver *s, int32_t world);
int saa_step_peer(saa_solver *s, int32_t nsteps, double *hist_dev, int64_t hist_row0);

/* nsteps sync-free steps of the predicted phase (Online_predictor.py:287-316): after each local
 * update the shared dofs are overwritten by row (table_row0 + k) of table_dev (row length
 * 3*n_shared, fp64) and recorded into row (hist_row0 + k) of hist_dev (may be NULL). */
int saa_step_predicted(saa_solver *s, int32_t nsteps, const double *table_dev, int64_t table_row0,
                       double *hist_dev, int64_t hist_row0);

/* Trajectory recorder: the ground-truth loop's `d1_save[:, counter] = d1` (Data_prepare.py:236-240; likewise
 * Online_predictor.py:316-318) without leaving the GPU.  traj_dev is a caller-owned DEVICE matrix, row-major
 * (3*n_nodes, n_cols) in the caller's dof order - the layout of the reference's `Displacement` dataset.  From now on
 * every step taken through this handle (any stepping entry point, resident kernel included) has a step index,
 * starting at next_step_index; the displacement d^(n+1) of step index i is written to column i / save_every
 * whenever i % save_every == 0 and that column exists.  traj_dev = NULL switches the recorder off. */
int saa_set_recorder(saa_solver *s, double *traj_dev, int64_t n_cols, int32_t save_every, int64_t next_step_index);

/* d_sol_shared[i,:] = d0[loc_dof_shared] (Online_predictor.py:260,301) / the reverse overwrite
 * (:298) on the CURRENT d0, for callers that drive single steps themselves. */
int saa_halo_gather(saa_solver *s, double *row_dev);
int saa_halo_scatter(saa_solver *s, const double *row_dev);

/* Whether saa_step / saa_step_predicted / saa_step_peer calls of >= 8 steps run through the resident multi-step
 * kernel (one launch per steps_per_launch steps, the partition's image kept in LDS between steps,
 * DESIGN.md section 4) and how much LDS a workgroup of it holds.  capable = 0: the plan does not fit or the device
 * cannot keep all workgroups co-resident; every step is then one launch of the fused kernel. */
int saa_resident_kernel_info(const saa_solver *s, int32_t *capable, int32_t *lds_bytes, int32_t *steps_per_launch);
/* enable = 0: keep this handle on one launch per step (for callers that know the device is shared with other
 * processes: workgroups of a resident kernel that wait for another process' kernel only advance by time-slicing). */
int saa_set_resident_kernel(saa_solver *s, int32_t enable);
/* Run-time options of a handle, by name (the library itself reads no environment variable):
 *   "synced_graph"    1 (default) / 0: saa_step_synced replays HIP graphs of three steps each / enqueues every kernel and
 *                     collective itself (the role of the per-step MPI calls of Distributed_tools.py:77-92);
 *   "split_stepping"  1 (default) / 0: partitions too large for the resident kernel (several rounds of workgroups per
 *                     launch) step their blocks as three sets on three streams, so that one set's launch boundaries hide
 *                     under another's work / one launch of all blocks per step;
 *   "wait_timeout_s"  bound, in seconds (default 30), of every in-kernel wait for another workgroup or rank (resident
 *                     kernel, peer exchange); a wait that gives up is reported as SAA_E_STATE by saa_synchronize.
 * The reference has no counterpart (an MPI rank that loses its peer hangs, Distributed_tools.py:77-92). */
int saa_set_option(saa_solver *s, const char *name, double value);

/* Deterministic mode.  The step kernels accumulate the element forces of a node with LDS floating-point atomics, whose
 * order is free: f_int - and with it the trajectory - differs in the last bits from run to run (the same class of
 * difference as the reference's own dependence on partition and node numbering).  enable = 1 switches
 * this handle to a two-kernel form of the step without atomics: every work item writes its force vectors to memory and every
 * node adds the vectors addressed to it in a fixed order.  Same arithmetic per element, bit-identical results from run to
 * run; several times slower (a verification mode).  Covers saa_step, saa_step_begin/finish, saa_step_synced,
 * saa_step_predicted and saa_internal_force*; saa_step_peer is refused while it is on. */
int saa_set_deterministic(saa_solver *s, int32_t enable);

/* Blocks until all work enqueued for this handle has finished. */
int saa_synchronize(saa_solver *s);

/* Measurement aid for bench.py: device-to-device copy rate of this GPU - bytes read + bytes written per second by a
 * 16-byte-per-lane copy kernel over two buffers of n_bytes each, `reps` timed launches - the practical HBM ceiling that
 * SURVEY.md section 8(d) asks to be reported next to the nominal peak.  No counterpart in the reference (which has no
 * timing code at all: BASELINE.md section 1). */
int saa_device_copy_bandwidth(int32_t device, int64_t n_bytes, int32_t reps, double *bytes_per_s);

/*
 * Partition bookkeeping of ONE rank on the GPU: what Data_prepare.py:104-144 derives from the element partition `epart`
 * (`recvbuf`, Data_prepare.py:97-101) through Tools/Distributed_tools.py - `rankwise_dist` (:14-24: the rank's elements
 * and its nodes in first-touch order), `find_shared_nodes` (:29-40) + `sort_shared` (:44-51: `shared_nodes`,
 * `Global_shared`), `local_mat_node` (:66-73: local connectivity), `Dirichlet_rank_dist` (:55-62) - and the clamp detection
 * of Data_prepare.py:127-136 (nodes of boundary facets with all |x| < tol), in the reference's orderings, as O(N) device
 * passes + radix sorts instead of O(N^2) list scans.  Host arrays in; the results are held by the handle until copied out.
 *   tets   (n_elems, 4) GLOBAL node ids of the whole mesh, epart (n_elems) part of every element, 0 <= rank < n_parts;
 *   xyz (n_nodes, 3) and facets (n_facets, 3) may be null / 0: no clamp detection then.
 * saa_topology_sizes fills sizes[6] = { elements, nodes, shared nodes of the rank, Global_shared, clamped nodes of the
 * mesh, clamped nodes of the rank }; saa_topology_get copies into caller buffers of those sizes (any pointer may be null):
 *   elements (ascending), nodes (first-touch order), cells_local (elements x 4, local ids), shared_nodes (global ids,
 *   find_shared_nodes' order), shared_local, shared_slots (position in Global_shared), global_shared (sorted),
 *   dirichlet_nodes (global ids, first-seen order over the facets), dirichlet_local (local ids, ascending).
 */
typedef struct saa_topology saa_topology;
int saa_topology_build(int32_t device, int32_t n_nodes, int32_t n_elems, const int32_t *tets, const int32_t *epart, int32_t rank,
                       int32_t n_parts, const double *xyz, int32_t n_facets, const int32_t *facets, double clamp_tol,
                       saa_topology **out);
int saa_topology_sizes(const saa_topology *t, int32_t *sizes);
int saa_topology_get(const saa_topology *t, int32_t *elements, int32_t *nodes, int32_t *cells_local, int32_t *shared_nodes,
                     int32_t *shared_local, int32_t *shared_slots, int32_t *global_shared, int32_t *dirichlet_nodes,
                     int32_t *dirichlet_local);
int saa_topology_destroy(saa_topology *t);

/*
 * Modal analysis: stable time step and vibration modes of one whole mesh on one GPU.  The handle owns the mesh on the device
 * in the caller's numbering (cells = global node ids, dof = 3*node + component) and is independent of the step plan.
 *
 * saa_operator_create: the mesh, the clamped dofs (`Dirichlet`, node_to_dof of Data_prepare.py:127-136) and the material
 *   (lambda, mu of `elasticity`, commons.py:25-31; rho).  Stands for the matrix pair `M, K, _ = Global_Assembly(deg, Cells,
 *   Points, Dirichlet, elas, t)` of Eigen_mode (Tools/Steady_solvers.py:25-27, Mat_construction.py:154-196) without the
 *   matrices.  At most 2^29 elements.
 * saa_operator_apply: KX and / or MX (either output may be NULL) for 1 <= m <= 16 column-major columns of 3*n_nodes dofs
 *   (leading dimensions ldx, ldy >= 3*n_nodes), device buffers, in one launch pair per product.  K is the element stiffness
 *   of Local_K_coronary (Mat_construction.py:79-119), M the consistent mass rho V/20 (1 + delta_ab) I_3 of Local_MKF
 *   (Mat_construction.py:23-76, the 4-point rule of Qudrature.py:6-12 integrates it exactly).  Dirichlet rows and columns
 *   are masked like Global_Assembly leaves them out (Mat_construction.py:176-192): inputs there are ignored, outputs there
 *   are 0.  Bitwise repeatable (nodal sums in ascending element order, no floating-point atomics); enqueued on the
 *   handle's stream.
 * saa_operator_element_bound: omega_e = sqrt(lambda_max(K_e) / (rho |V_e| / 4)) of every element (omega_e_dev: n_elems
 *   doubles, may be NULL), their maximum, its element and the number of elements whose signed volume (detJ / 6,
 *   Mat_construction.py:93) is <= 0.  2 / omega_max bounds the stable step of the central-difference update
 *   (Dynamic_solver.py:13-20, lumped mass of commons.py:103-107) from below only when that number is 0.  Synchronises the
 *   handle's stream.  No counterpart in the reference, whose step comes from the edge-length rule (commons.py:79-90,
 *   Data_prepare.py:147).
 *
 * The same handle serves stress recovery (saa_operator_stress, saa_operator_nodal_average, saa_operator_stress_error,
 * below), with the geometry of the K apply.  The reference has no counterpart: it stores displacement only.
 *
 * Quadratic tetrahedra (p = 2, the reference's second element: `Global_Assembly(2, ...)`, n_basis = 10).
 * saa_operator_create_p2: as saa_operator_create with 10 node ids per element in the reference's local order
 *   (Shape_function_Deriv.py:14-23, VTK cell type 24): the four vertices, then the nodes on the edges (0,1), (1,2), (0,2),
 *   (0,3), (1,3), (2,3).  The geometry is isoparametric: the Jacobian comes from all ten nodes at every quadrature point
 *   (Shape_function_Deriv.py:60-67), so curved elements are legal; detJ is signed.  At most 214 748 364 elements
 *   (10 * n_elems + corner must fit 32 bits).
 * saa_operator_order: 1 or 2.
 * saa_operator_apply on an order-2 handle means the same: 1..16 columns, Dirichlet rows and columns masked, bitwise
 *   repeatable without floating-point atomics, every column independent of the others in the call.  K uses the reference's
 *   rule for deg == 2 (n_quad = 2: the 4-point rule, Mat_construction.py:84-89).  M uses the 14-point rule Gauss_Legendre(4)
 *   and NOT the reference's 4-point rule: a DELIBERATE DEVIATION.  With four points the 30 x 30 element mass has rank 12
 *   and the assembled mass is singular (36-tet 6 x 1 x 1 beam: 18 of 351 eigenvalues are 0, the smallest is -1e-17), so the
 *   reference's own Eigen_mode(2, ...) cannot work; the 14-point mass is positive definite on the same mesh (smallest
 *   eigenvalue 3.3e-3) and its total is exact.
 * saa_operator_load (either order): the consistent body-force vector sum_q w_q detJ_q N_a(xi_q) (fx, fy, fz) with the K rule,
 *   `Fe` of Local_MKF assembled (the reference's load is (0, -fz, -fz), commons.py:35-41); 3*n_nodes doubles on the device,
 *   0 on Dirichlet dofs.
 * saa_operator_diagonal (either order): diag(K) and / or diag(M) of the masked operator (0 on Dirichlet dofs), 3*n_nodes
 *   doubles each on the device, either may be NULL - what a Jacobi preconditioner needs.  Order 1: the closed form of
 *   Local_K_coronary's diagonal and rho V / 10.
 * saa_operator_element_bound, saa_operator_stress, saa_operator_nodal_average and saa_operator_stress_error are formulas of
 *   the linear element: on an order-2 handle they return SAA_E_ARG, say so in saa_last_error and launch nothing.  The
 *   stress of an order-2 handle comes from saa_operator_stress_p2, saa_operator_nodal_stress_p2 and
 *   saa_operator_stress_error_p2 (below, after the linear ones), which in turn refuse an order-1 handle.
 */
typedef struct saa_operator saa_operator;
int saa_operator_create(int32_t device, int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *tets,
                        const int32_t *dirichlet_dofs, int32_t n_dirichlet, double lambda_, double mu, double rho,
                        saa_operator **out);
int saa_operator_create_p2(int32_t device, int32_t n_nodes, int32_t n_elems, const double *xyz, const int32_t *cells10,
                           const int32_t *dirichlet_dofs, int32_t n_dirichlet, double lambda_, double mu, double rho,
                           saa_operator **out);
int saa_operator_order(const saa_operator *op);
int saa_operator_load(saa_operator *op, double fx, double fy, double fz, double *f_dev);
int saa_operator_diagonal(saa_operator *op, double *diag_k_dev, double *diag_m_dev);
/* All later work of this handle goes to `hip_stream` (a hipStream_t; NULL = null stream). */
int saa_operator_set_stream(saa_operator *op, void *hip_stream);
int saa_operator_apply(saa_operator *op, int32_t m, const double *x_dev, int64_t ldx, double *kx_dev, double *mx_dev,
                       int64_t ldy);
int saa_operator_element_bound(saa_operator *op, double *omega_e_dev, double *omega_max, int32_t *argmax,
                               int32_t *n_nonpositive);
/*
 * Stress recovery.  eps_e = sum_a B_a u_a (rows xx, yy, zz, yz, xz, xy, engineering shear: Mat_construction.py:99-104),
 * sigma_e = D eps_e (commons.py:25-31), von Mises vm_e, strain energy W_e = |V_e| sigma_e . eps_e / 2 with V_e = detJ / 6
 * (on a consistently oriented mesh sum_e W_e = d^T K d / 2).  The Dirichlet mask is not applied: x is read as given.
 * Bitwise repeatable (fixed-order reductions, no floating-point atomics); enqueued on the handle's stream, no host sync.
 *
 * saa_operator_stress: m in 1..16 column-major displacement columns (x: 3*n_nodes per column, ldx >= 3*n_nodes).  Outputs
 *   column-major, any may be NULL: sigma (6*n_elems per column, element e component c at 6e+c, ld_sigma >= 6*n_elems);
 *   von_mises and energy (n_elems per column, ld_elem >= n_elems); energy_total, von_mises_max (m doubles),
 *   von_mises_argmax (m int32: the lowest element index on ties).
 * saa_operator_nodal_average: volume-weighted nodal average sum_{e at v} |V_e| f_e / sum_{e at v} |V_e| (ascending element
 *   order; 0 at a node with no element) of k in 1..8 components per element: elem (k*n_elems per column, e*k+c,
 *   ld_elem >= k*n_elems), node (k*n_nodes per column, v*k+c, ld_node >= k*n_nodes).
 */
int saa_operator_stress(saa_operator *op, int32_t m, const double *x_dev, int64_t ldx, double *sigma_dev, int64_t ld_sigma,
                        double *von_mises_dev, double *energy_dev, int64_t ld_elem, double *energy_total_dev,
                        double *von_mises_max_dev, int32_t *von_mises_argmax_dev);
int saa_operator_nodal_average(saa_operator *op, int32_t m, int32_t k, const double *elem_dev, int64_t ld_elem, double *node_dev,
                               int64_t ld_node);
/*
 * Stress error per element in the energy norm, with the compliance C = D^-1 (engineering shear):
 *   eta_e^2 = integral_e (sigma_A - sigma_e)^T C (sigma_A - sigma_e) dV,
 * sigma_e the element stress (sigma_elem: 6*n_elems per column, 6e+c, ld_sigma >= 6*n_elems) and sigma_A exactly one of
 *   sigma_node: nodal values (6*n_nodes per column, 6v+c, ld_node >= 6*n_nodes), interpolated linearly over the element.
 *     With the nodal average of sigma_e this is the Zienkiewicz-Zhu estimate; the integral is exact:
 *     eta_e^2 = |V_e| / 20 (s^T C s + sum_a delta_a^T C delta_a), delta_a = sigma_A(vertex a) - sigma_e, s = sum_a delta_a;
 *   sigma_other: a second element field (6*n_elems per column, 6e+c, ld_other >= 6*n_elems): eta_e^2 = |V_e| delta^T C delta.
 * The other one is NULL.  m in 1..16 columns.  Outputs, any may be NULL (all NULL: nothing is launched): eta2 (n_elems per
 * column, ld_eta >= n_elems); eta2_total, eta2_max (m doubles), eta2_argmax (m int32: the lowest element index on ties; -1
 * and 0.0 on a mesh without elements).  Needs mu > 0 and 3 lambda + 2 mu > 0.  Bitwise repeatable (fixed-order reductions, no
 * floating-point atomics), a column's results do not depend on the other columns of the call; enqueued on the handle's
 * stream, no host sync.  No counterpart in the reference.
 */
int saa_operator_stress_error(saa_operator *op, int32_t m, const double *sigma_elem_dev, int64_t ld_sigma,
                              const double *sigma_node_dev, int64_t ld_node, const double *sigma_other_dev, int64_t ld_other,
                              double *eta2_dev, int64_t ld_eta, double *eta2_total_dev, double *eta2_max_dev,
                              int32_t *eta2_argmax_dev);
/*
 * Stress recovery and error estimate of the quadratic element, on an order-2 handle (saa_operator_create_p2).  Voigt rows,
 * D, fp64, repeatability and the stream as above; the Dirichlet mask is not applied.  The Gauss points q = 0..3 are those
 * of the K rule, Gauss_Legendre(2): point q has barycentric weight a = 0.5854101966249685 on vertex v(q) = 1, 2, 3, 0 and
 * b = 0.1381966011250105 on the others (q(v) = 3, 0, 1, 2 is the inverse).  All three take m in 1..16 column-major columns;
 * any output may be NULL, and with every output NULL nothing is launched.  On an order-1 handle they return SAA_E_ARG, name
 * themselves and "order-1" in saa_last_error and launch nothing.  No counterpart in the reference.
 *
 * saa_operator_stress_p2: eps_q = sum_a B_a(xi_q) u_a with the isoparametric gradients of the K apply, sigma_q = D eps_q,
 *   its von Mises value, W_e = 1/2 sum_q w_q |detJ_q| sigma_q . eps_q (where every detJ_q > 0, sum_e W_e = x^T K x / 2 of a
 *   handle without Dirichlet dofs).  x: 3*n_nodes per column, ldx >= 3*n_nodes.  sigma: 24*n_elems per column, 24e+6q+c,
 *   ld_sigma >= 24*n_elems; von_mises: 4*n_elems per column, 4e+q, ld_vm >= 4*n_elems; energy: n_elems per column,
 *   ld_elem >= n_elems; energy_total, von_mises_max (m doubles), von_mises_argmax (m int32: the point index 4e+q, the
 *   lowest on ties).
 * saa_operator_nodal_stress_p2: the recovered nodal stress.  The field that is linear in the barycentric coordinates and
 *   takes the four Gauss values has the vertex values c_v = sqrt(5) (sigma_q(v) - b S), S = sum_q sigma_q; an edge node
 *   takes the mean of its two vertices.  On a straight element this field is the finite-element stress itself; on a curved
 *   one it is the definition of the element stress sigma_h used here and below (a DELIBERATE simplification: the
 *   finite-element stress of a curved element is rational in xi).  sigma_node[6n+c] = sum_{e at n} |V_e| c_{e,corner(n)} /
 *   sum_{e at n} |V_e| with |V_e| = sum_q w_q |detJ_q|, ascending element order, 0 at a node with no element; 6*n_nodes
 *   per column, ld_node >= 6*n_nodes.
 * saa_operator_stress_error_p2: eta_e^2 = integral_e d^T C d dV, C = D^-1 (needs mu > 0 and 3 lambda + 2 mu > 0), against
 *   exactly one of sigma_node (6*n_nodes per column: d = sum_a N_a sigma_node_a - sigma_h with the ten quadratic shape
 *   functions, integrated with the 14-point rule Gauss_Legendre(4) and |detJ| at its points, exact on straight elements;
 *   with saa_operator_nodal_stress_p2 of sigma this is the Zienkiewicz-Zhu estimate) and sigma_other (a second Gauss-point
 *   field, 24*n_elems per column, ld_other >= 24*n_elems: d_q = sigma_other_q - sigma_q with the 4-point rule, exact on
 *   straight elements).  The other one is NULL.  eta2: n_elems per column, ld_eta >= n_elems; eta2_total, eta2_max (m
 *   doubles), eta2_argmax (m int32: the lowest element index on ties; -1 and 0.0 on a mesh without elements).
 */
int saa_operator_stress_p2(saa_operator *op, int32_t m, const double *x_dev, int64_t ldx, double *sigma_dev, int64_t ld_sigma,
                           double *von_mises_dev, int64_t ld_vm, double *energy_dev, int64_t ld_elem, double *energy_total_dev,
                           double *von_mises_max_dev, int32_t *von_mises_argmax_dev);
int saa_operator_nodal_stress_p2(saa_operator *op, int32_t m, const double *sigma_dev, int64_t ld_sigma, double *sigma_node_dev,
                                 int64_t ld_node);
int saa_operator_stress_error_p2(saa_operator *op, int32_t m, const double *sigma_dev, int64_t ld_sigma,
                                 const double *sigma_node_dev, int64_t ld_node, const double *sigma_other_dev, int64_t ld_other,
                                 double *eta2_dev, int64_t ld_eta, double *eta2_total_dev, double *eta2_max_dev,
                                 int32_t *eta2_argmax_dev);
int saa_operator_destroy(saa_operator *op);

/*
 * Explicit dynamics on the operator handle, either order: the time loop of Data_prepare.py:215-240 for one whole mesh on one
 * GPU.  The reference stops before it for its second element ("p=2 only works for steady case, dynamic case requires
 * advanced lumping method", Data_prepare.py:43; "dynamics problem for p=2 TBD", Mat_construction.py:31).  All pointers are
 * device pointers; work is enqueued on the operator's stream with no host synchronisation unless stated; no floating-point
 * atomics, bitwise repeatable.
 *
 * saa_operator_lumped_mass: 3*n_nodes doubles, one value on a node's three dofs; the Dirichlet mask is NOT applied (the mass
 *   stays positive there).  Order 2 is HRZ lumping, because the reference's row sum (lumping_to_vec, commons.py:103-107)
 *   gives every vertex of a quadratic tetrahedron the negative mass rho integral N_vertex = -rho V/20: per element
 *   m_a = rho (sum_q w_q detJ_q) I_a / sum_b I_b with I_a = sum_q w_q detJ_q N_a(xi_q)^2 over the 14-point rule (on a straight
 *   element rho V/36 at a vertex, 4 rho V/27 on an edge), summed over a node's elements in ascending element order.  Order 1
 *   is the row sum rho V_e / 4 per vertex (V_e = detJ / 6, signed): the lumped mass of saa_setup_fields.
 * saa_operator_stepper_create: a stepper that BORROWS the operator (which must outlive it, and whose stream it uses) and
 *   copies the mass and the un-ramped load (3*n_nodes each); state d0 = dn = 0, tn = 0.  SAA_E_ARG on null pointers,
 *   dt <= 0, alpha < 0, or a mass that is not > 0 at a node that has elements (checked once; synchronises the stream).
 *   The edge-length rule of Data_prepare.py:147 is NOT a stable dt for the quadratic element (1.56 x 2/omega_max on the
 *   36-tet beam): take dt from omega_max of M_L^-1 K (modal.stable_time_step_operator).
 * saa_operator_stepper_step: nsteps (0: nothing) steps of Dynamic_solver.py:12-20 on one rank,
 *     f_int = K d0 (masked operator),  f_ext = f * (ramp ? min(tn, 1) : 1),
 *     d1 = (dt^2 (f_ext - f_int) + 2 m d0 - m dn + dt/2 m alpha dn) / (m + alpha m dt / 2),  d1[Dirichlet] = 0,  tn += dt,
 *   d1 = 0 at a node that has no element (whatever its mass).  Two launches per step: the K element pass for one column
 *   and a node pass fused with the update, which overwrites dn (the state is two buffers and a swap); f_int is never
 *   written to memory.  On an order-1 handle this is NOT a rival of saa_step, whose kernel keeps the partition in LDS over
 *   several steps: it exists so that one stepper serves both orders and saa_step is a second oracle for it.
 * saa_operator_stepper_set_state: d0 = d^n, dn = d^(n-1) (NULL = zeros), tn.  saa_operator_stepper_get_state: into
 *   caller buffers (either may be NULL); synchronises the stream.
 * saa_operator_stepper_set_recorder: exactly saa_set_recorder - row-major (3*n_nodes, n_cols), the d^(n+1) of step index i
 *   goes to column i / save_every whenever i % save_every == 0 and that column exists; NULL switches it off.
 * saa_operator_stepper_set_option: "stored_geometry" 0 (default) / 1 - the order-2 element pass rebuilds J^-1 and w detJ at
 *   its four points from the thirty gathered coordinates every step / reads them from a table built once, 40 doubles per
 *   element stored component-major (profiles/p2_step_kernel_stats.txt has the comparison).  No effect on order 1.
 *   "passes" 3 (default) / 1 / 2 is a measurement aid for tools/p2_step_point.py: a step launches both passes / the element
 *   pass only / the node pass only; the state and tn advance only with 3.
 */
int saa_operator_lumped_mass(saa_operator *op, double *mass_dev);
typedef struct saa_operator_stepper saa_operator_stepper;
int saa_operator_stepper_create(saa_operator *op, const double *mass_dev, const double *f_ext_dev, double dt, double alpha,
                                int32_t ramp, saa_operator_stepper **out);
int saa_operator_stepper_set_state(saa_operator_stepper *st, const double *d0_dev, const double *dn_dev, double tn);
int saa_operator_stepper_get_state(saa_operator_stepper *st, double *d0_dev, double *dn_dev, double *tn);
int saa_operator_stepper_set_recorder(saa_operator_stepper *st, double *traj_dev, int64_t n_cols, int32_t save_every,
                                      int64_t next_step_index);
int saa_operator_stepper_set_option(saa_operator_stepper *st, const char *name, double value);
int saa_operator_stepper_step(saa_operator_stepper *st, int32_t nsteps);
int saa_operator_stepper_destroy(saa_operator_stepper *st);

/*
 * The operator stepper on one rank of a partition, either order: the synchronised step (MODEL=False, Dynamic_solver.py:22-32)
 * split around the caller's reduction of the shared-node forces, the predicted step with the shared-dof overwrite
 * (Online_predictor.py:287-316) and the gather / scatter of the shared dofs.  The meaning is that of saa_step_begin,
 * saa_step_finish, saa_step_predicted, saa_halo_gather and saa_halo_scatter on the linear solver handle.  Device pointers
 * except where marked host; enqueued on the operator's stream with no host synchronisation (set_shared synchronises); no
 * floating-point atomics, bitwise repeatable.
 *
 * saa_operator_stepper_set_shared: shared_local_host[k] is the local node id of this rank's k-th shared node,
 *   shared_slots_host[k] its position in the sorted Global_shared of n_global_shared nodes; a table or history row is
 *   3*n_shared doubles in that order (loc_dof_shared).  SAA_E_ARG on ids or slots out of range or repeated, or
 *   n_shared > n_global_shared.  n_shared = 0 clears the rank's shared set (with n_global_shared > 0 every slot is foreign).
 *   Builds on the device the map node -> k (-1 for a node that is not shared), the lists of nodes and slots, and the list
 *   of foreign slots: those of Global_shared that this rank does not hold.  Switches the energy balance off
 *   (saa_operator_stepper_set_energy, below): call that after this.
 * saa_operator_stepper_set_interface_buffer: 3*n_global_shared doubles, caller-owned, zero when handed over.
 * saa_operator_stepper_step_begin: the K element pass for d0 (the variant "stored_geometry" selects) and one node pass.  A
 *   node that is not shared is updated and recorded as saa_operator_stepper_step does it.  A shared node's contributions,
 *   summed in ascending element order, go to iface[3*slot + c]; its dn entry is left alone: d1 overwrites dn in place in
 *   this stepper, so unlike the linear kernel there is no provisional update of shared nodes.  The stepper is then pending.
 * saa_operator_stepper_step_finish: one launch over the shared dofs and the foreign slots.  d1 from iface[3*slot + c] - by
 *   now the sum over the ranks -, the stepper's mass and load, d0, dn and the step's ramp, by the same device function as the
 *   node pass; 0 on a Dirichlet dof; written over dn, into the recorder column and into
 *   hist_dev[hist_row*3*n_shared + 3k + c] when hist_dev is not NULL.  Foreign slots are zeroed again.  Then the buffers
 *   swap, tn += dt and the step index advances.
 * saa_operator_stepper_step_predicted: nsteps steps of two launches each.  Shared dofs take
 *   table_dev[(table_row0 + k)*3*n_shared + ...] unconditionally, on a Dirichlet dof too (Online_predictor.py:298); the value
 *   also goes to row hist_row0 + k of hist_dev (NULL: none) and to the recorder.  Other nodes as saa_operator_stepper_step.
 * saa_operator_stepper_halo_gather / _halo_scatter: row_dev[3k + c] <-> the current d0 at the shared dofs.
 * saa_operator_stepper_step is unchanged: with a shared set it is the local step without overwrite (MODEL=True).  The
 *   begin / finish / predicted steps ignore the "passes" measurement option.
 * SAA_E_STATE: step_finish without step_begin; step, step_predicted, step_begin, set_state, set_recorder, set_option,
 *   set_shared, set_interface_buffer, halo_scatter while pending; step_begin with n_global_shared > 0 and no interface
 *   buffer.  SAA_E_ARG: null handle, negative nsteps or rows, a null table or row with n_shared > 0.
 */
int saa_operator_stepper_set_shared(saa_operator_stepper *st, int32_t n_shared, const int32_t *shared_local_host,
                                    const int32_t *shared_slots_host, int32_t n_global_shared);
int saa_operator_stepper_set_interface_buffer(saa_operator_stepper *st, double *iface_dev);
int saa_operator_stepper_step_begin(saa_operator_stepper *st);
int saa_operator_stepper_step_finish(saa_operator_stepper *st, double *hist_dev, int64_t hist_row);
int saa_operator_stepper_step_predicted(saa_operator_stepper *st, int32_t nsteps, const double *table_dev, int64_t table_row0,
                                        double *hist_dev, int64_t hist_row0);
int saa_operator_stepper_halo_gather(saa_operator_stepper *st, double *row_dev);
int saa_operator_stepper_halo_scatter(saa_operator_stepper *st, const double *row_dev);

/*
 * The energy balance of the operator stepper: what says whether a run is healthy.  Write d1 = d^(n+1), d0 = d^n, dn = d^(n-1),
 * s = K d0 (the internal force, which the node pass holds in registers and never writes) and lambda_n = ramp ? min(t_n, 1) : 1.
 * The update of saa_operator_stepper_step is  m (d1 - 2 d0 + dn)/dt^2 + alpha m (d1 - dn)/(2 dt) + s = lambda_n f.  Multiplied
 * by (d1 - dn)/2 and summed over the dofs it gives, with the symmetry of K and exactly in the discrete sense,
 *     (T + U)_{n+1/2} - (T + U)_{n-1/2} = dW_n - dD_n,   where
 *     T_{n+1/2} = 1/2 sum_i m_i ((d1_i - d0_i)/dt)^2          kinetic energy of the half step
 *     U_{n+1/2} = 1/2 sum_i d1_i s_i                          strain energy in cross form, 1/2 d^(n+1) . K d^n
 *     U_n       = 1/2 sum_i d0_i s_i                          strain energy at t_n
 *     dW_n      = lambda_n sum_i f_i (d1_i - dn_i)/2          work of the ramped load
 *     dD_n      = alpha/(4 dt) sum_i m_i (d1_i - dn_i)^2      loss to the mass-proportional damping
 * so that with the running sums W_{n+1} = sum_{j<=n} dW_j and D_{n+1} = sum_{j<=n} dD_j
 *     B_n = T_{n+1/2} + U_{n+1/2} - W_{n+1} + D_{n+1}
 * is constant to round-off over whole-mesh and synchronised steps from the step at which recording began.  B measures the
 * CONSISTENCY of the run, not its stability: above the stability limit T + U grows without bound while B stays constant,
 * so watch both.  In a predicted window the shared dofs are overwritten and the drift of B is the work done through the
 * interface - the energy the predictor injects -, an error figure that needs no synchronised run to compare with.
 * A Dirichlet dof and a node without elements contribute 0 to every sum.
 *
 * saa_operator_stepper_set_energy: energy_dev is a row-major (n_rows, 5) device buffer with the columns T_{n+1/2}, U_{n+1/2},
 *   U_n, W_{n+1}, D_{n+1}; by the recorder's rule the step with energy step index i (next_step_index at this call, + 1 per
 *   step, a counter of its own) writes row i / every when i % every == 0 and that row exists.  W and D are summed on the
 *   device over EVERY step since this call, which zeroes them.  energy_dev = NULL switches the balance off.  While it is on,
 *   step, step_begin / step_finish and step_predicted launch energy variants of the node and finish passes - the same
 *   update by the same device function, the state bit-equal to a run with the balance off - which reduce the five sums per
 *   block, and one more one-block launch per step that sums the blocks' partials in a fixed order.  No floating-point
 *   atomics: every figure is bitwise repeatable and independent of how a run is split into calls.  While it is off exactly
 *   the kernels of a stepper that never had it are launched.
 *   One rank of a partition records its SHARE: the rows of all ranks add up to the row of the whole mesh.  The terms with m
 *   or f (T, dW, dD) carry the global mass and load, which every holder of a shared node has in full, so a shared node
 *   counts only on the rank with shared_owned_host[k] != 0 (n_shared host bytes in the order of shared_local_host; NULL:
 *   all owned; give every shared node to exactly one of its holders, e.g. the lowest).  U_n is formed on every holder from
 *   its partial s, and the partial s add up.  U_{n+1/2} of a shared node is formed in a synchronised step by the owner from
 *   the summed s of the interface buffer, in a predicted step by every holder from its partial s and the d1 of its own
 *   table.  saa_operator_stepper_step on a stepper with a shared set counts every node of the rank as owned.
 *   SAA_E_ARG, before the handle or the device is looked at: n_rows < 0, every < 1, next_step_index < 0; then a null handle.
 *   SAA_E_STATE: between step_begin and step_finish; with the "passes" option at 1 or 2 (and that option is refused while
 *   the balance is on).  Synchronises the stream.  saa_operator_stepper_set_shared switches the balance OFF, because the
 *   ownership flags and the partial sums are sized by the shared set: call set_energy after it.
 */
int saa_operator_stepper_set_energy(saa_operator_stepper *st, double *energy_dev, int64_t n_rows, int32_t every,
                                    int64_t next_step_index, const uint8_t *shared_owned_host);

/*
 * Finite-strain hyperelastic materials on the operator handle, either element order (csrc/saa_opfs.hip).  Every other kernel
 * of the handle is small-strain linear elasticity, sigma = lambda tr(H) I + mu (H + H^T), whose internal force does not
 * vanish under a rigid rotation - and a slender cantilever in bending rotates.  Total-Lagrangian: with H = grad_X u and
 * F = I + H at the points of the K rule (order 1: the one constant gradient; order 2: the four Gauss points, H formed as the
 * linear pass forms it) the first Piola-Kirchhoff stress P takes the place of sigma,
 *     f_a[i] = sum_q w_q detJ_q sum_k P_q[i][k] dN_a/dX_k(q),
 * with the sign and detJ convention of the linear pass of the same order and u masked to 0 on Dirichlet dofs on input.  Both
 * materials take the handle's lambda and mu and linearise to the handle's K at u = 0:
 *   SAA_MATERIAL_SVK          St. Venant-Kirchhoff: E = (H + H^T + H^T H)/2, S = lambda tr(E) I + 2 mu E, P = F S,
 *                             W = lambda/2 tr(E)^2 + mu E:E
 *   SAA_MATERIAL_NEO_HOOKEAN  compressible neo-Hooke: J = det F, P = mu (F - F^-T) + lambda ln(J) F^-T,
 *                             W = mu/2 (F:F - 3) - mu ln J + lambda/2 (ln J)^2
 * Inversion.  Under neo-Hooke an element with !(J > 0) at any of its points (NaN included) contributes 0 from all its corners
 * for that evaluation and is counted; SVK does not look at J.  The counters are two device words updated with integer
 * atomics.  There are no floating-point atomics: every result is bitwise repeatable and independent of how a run is split
 * into calls.  The order-2 passes read the reduced geometry table of the "stored_geometry" option (40 doubles and one word
 * per element), which the HANDLE owns: it is made on first need by whoever asks - this call, a stepper with that option or
 * with a nonlinear material -, there is one per handle, and saa_operator_destroy frees it.  There is no recomputing
 * variant of the order-2 finite-strain pass.
 *
 * saa_operator_internal_force: f_dev = f_int(x_dev), one column of 3*n_nodes doubles, 0 on Dirichlet dofs: the element pass
 *   and the node sum of saa_operator_apply.  material = SAA_MATERIAL_LINEAR runs the kernels of saa_operator_apply with
 *   m = 1 (bit-equal to it).  energy_elem_dev (n_elems doubles or NULL) = sum_q w_q |detJ_q| W(F_q) per element, 0 for an
 *   inverted one; with the linear material it is refused (saa_operator_stress has that energy).  n_inverted (host, or NULL)
 *   = the number of inverted elements of this call; asking for it synchronises the stream, otherwise the call is enqueued.
 *   SAA_E_ARG, before the handle or the device is looked at: a material outside {0, 1, 2}; then a null handle, null x_dev or
 *   f_dev, energy_elem_dev with material 0.
 * saa_operator_stepper_set_material: the element pass of step, step_begin and step_predicted becomes that of `material`;
 *   the node passes, the shared-node split, the recorder and the update are what they were, since they only sum whatever
 *   the element pass wrote.  SAA_MATERIAL_LINEAR (the default) restores the linear pass that "stored_geometry" selects, and
 *   then exactly the kernels of a stepper that never had a material are launched; that option governs the linear pass only.
 *   Clears the inversion counters.  SAA_E_ARG as above; SAA_E_STATE between step_begin and step_finish, and while the energy
 *   balance is on.  saa_operator_stepper_set_energy in turn returns SAA_E_STATE while a nonlinear material is set: its
 *   identity needs a symmetric constant K, and a balance for W(F) is not provided.
 *   THE TIME STEP IS NOT FOLLOWED: dt stays what the stepper was created with, by convention gamma * 2/omega_max of the
 *   LINEAR operator at the reference configuration.  Under large stretch the tangent stiffens and the stability limit
 *   moves below that; watch the displacements (and, under neo-Hooke, the inversion counters).  The limit at a state can
 *   be MEASURED: 2/omega_max of M_L^-1 K_T(d) by Lanczos on saa_operator_tangent_apply (modal.stable_time_step_operator,
 *   OperatorStepper.stable_time_step, drivers dynamics --dt-check-every); the stepper never changes the step by itself.
 *   A caller can FOLLOW the limit with saa_operator_tangent_bound and saa_operator_stepper_set_dt (below;
 *   OperatorStepper.follow_time_step, drivers dynamics --dt-follow).
 * saa_operator_tangent_apply: kv_dev = K_T(u_dev) v_dev, the tangent of saa_operator_internal_force at u applied to one
 *   column v, K_T(u) v = d/ds f_int(u + s v) at s = 0 (csrc/saa_optan.hip): one column of 3*n_nodes doubles, 0 on Dirichlet
 *   dofs.  u and v are both masked to 0 on Dirichlet dofs on input, exactly as saa_operator_internal_force masks x.  At each
 *   point of the K rule, with H = grad_X u and dH = grad_X v formed as the force pass forms H and its weights and sign:
 *     SAA_MATERIAL_SVK          dE = (dH + dH^T + H^T dH + dH^T H)/2, dS = lambda tr(dE) I + 2 mu dE, dP = dH S + F dS
 *     SAA_MATERIAL_NEO_HOOKEAN  dP = mu dH + (mu - lambda ln J) F^-T dH^T F^-T + lambda (F^-T : dH) F^-T, with F^-T - I and
 *                               ln J from H as the force pass has them (cofactors of H, log1p(J - 1)), never from an
 *                               inverse of I + H
 *   and kv_a[i] = sum_q w_q detJ_q sum_k dP_q[i][k] dN_a/dX_k(q).  At u = 0 both are the handle's K; K_T is symmetric.
 *   SAA_MATERIAL_LINEAR runs the kernels of saa_operator_apply with m = 1 on v (bit-equal to it); u_dev may then be NULL.
 *   Inversion: under neo-Hooke an element with !(J > 0) at any point, NaN included, contributes 0 from all its corners and is
 *   counted, by the rule and in the counter words of the force pass; SVK does not look at J.  n_inverted (host, or NULL) =
 *   that count; asking for it synchronises the stream, otherwise the call is enqueued.  The call uses the element
 *   contributions scratch and the node sum of the force; H(u) is recomputed on every call and nothing is stored per point.
 *   No floating-point atomics: bitwise repeatable.  SAA_E_ARG, before the handle or the device is looked at: a material
 *   outside {0, 1, 2}; then a null handle, null v_dev or kv_dev, null u_dev with a nonlinear material.
 * saa_operator_tangent_apply_block: the same operator on 1 <= m <= 16 column-major columns of 3*n_nodes dofs in one call
 *   (csrc/saa_optan_block.hip): column j of kv_dev (leading dimension ldkv) = K_T(u_dev) applied to column j of v_dev
 *   (leading dimension ldv), both leading dimensions >= 3*n_nodes as for saa_operator_apply.  Every column is defined exactly
 *   as above - the same point law, H and dH, weights, sign and masks - and does not depend on m, on the other columns of the
 *   call or on its place among them; it is a different kernel from the one-column entry, so the two agree to round-off, not
 *   bit for bit.  What does not depend on the column is done once per call: at order 1 the element's gradients, H(u) and the
 *   state of the point law are formed once per element and the columns loop inside the lane; at order 2 (the one-column pass
 *   already fills the register file) the column is the second grid index and each recomputes its element's state, so there
 *   the call saves launches and shares the one node sum over all columns.  Nothing is stored per point between calls.  The
 *   element pass writes m columns of the contributions scratch, which the node sum of saa_operator_apply adds up; no
 *   floating-point atomics, bitwise repeatable.  SAA_MATERIAL_LINEAR runs the K kernels of saa_operator_apply on the m
 *   columns (bit-equal to it); u_dev may then be NULL.  Inversion as above, for all columns at once: the element contributes
 *   0 to every column and is counted once per call, not once per column.  n_inverted (host, or NULL) = that count; asking for
 *   it synchronises the stream, otherwise the call is enqueued.  SAA_E_ARG, before the handle or the device is looked at: a
 *   material outside {0, 1, 2}, m outside 1..16, a negative ldv or ldkv; then a null handle, null v_dev or kv_dev, null u_dev
 *   with a nonlinear material, a leading dimension below 3*n_nodes.  Its user is modal.prestressed_modes, the natural
 *   frequencies of a loaded structure about its equilibrium, K_T(u*) x = omega^2 M x (drivers modal --material).
 * saa_operator_stepper_inverted: count = the number of (element, step) inversion events since the counters were cleared,
 *   first_step = the lowest step index (the recorder's, saa_operator_stepper_set_recorder) at which one occurred, -1 when
 *   none did.  set_material and set_state clear them.  Synchronises the stream.  Either output may be NULL.
 */
#define SAA_MATERIAL_LINEAR 0
#define SAA_MATERIAL_SVK 1
#define SAA_MATERIAL_NEO_HOOKEAN 2
int saa_operator_internal_force(saa_operator *op, int32_t material, const double *x_dev, double *f_dev,
                                double *energy_elem_dev /* n_elems or NULL */, int64_t *n_inverted /* or NULL */);
int saa_operator_tangent_apply(saa_operator *op, int32_t material, const double *u_dev, const double *v_dev,
                               double *kv_dev, int64_t *n_inverted /* host, or NULL */);
int saa_operator_tangent_apply_block(saa_operator *op, int32_t material, const double *u_dev /* NULL allowed with LINEAR */,
                                     int32_t m, const double *v_dev, int64_t ldv, double *kv_dev, int64_t ldkv,
                                     int64_t *n_inverted /* host, or NULL */);
int saa_operator_stepper_set_material(saa_operator_stepper *st, int32_t material);
int saa_operator_stepper_inverted(saa_operator_stepper *st, int64_t *count, int64_t *first_step /* -1: none */);

/*
 * Following the stable time step at finite strain (csrc/saa_opdt.hip).  Under stretch the tangent stiffens and the limit
 * 2/omega_max of M_L^-1 K_T(d) moves below the step a stepper was created with; these two entries let a caller recompute the
 * step as it runs - a one-pass element bound of omega_max at a state, and an exact change of dt between two steps.  Nothing
 * else of the stepper changes: a caller that uses neither launches exactly the kernels it launched before.
 *
 * saa_operator_tangent_bound: omega_e, an upper bound per element of the highest frequency at the state u, on a handle of
 *   either order and for all three materials; SAA_MATERIAL_LINEAR is the St. Venant-Kirchhoff law at H = 0 and u_dev is then
 *   not read (it may be NULL).  One element per lane; at each point q of the K rule (order 1: one; order 2: the four Gauss
 *   points) H = grad_X u is formed exactly as the force pass of that order forms it, u masked to 0 on Dirichlet dofs (order 2
 *   reads the handle's geometry table, made on first need).  With g_a = grad_X N_a(q) and m_a the element's share of the
 *   handle's lumped mass (order 1: rho |V_e| / 4; order 2: the HRZ share of saa_operator_lumped_mass):
 *     C_q = sum_a g_a g_a^T / m_a = R R^T (3x3, Cholesky),   A_q = dP/dF at H, the 9x9 symmetric material tangent (never stored),
 *     T_q = (I_3 (x) R)^T A_q (I_3 (x) R), built from nine evaluations of the point law of saa_operator_tangent_apply,
 *     mu_q = w_q |detJ_q| max(lambda_max(T_q), 0) by cyclic Jacobi in registers,   omega_e = sqrt(sum_q mu_q).
 *   max_e omega_e >= omega_max(M_L^-1 K_T(u)): the Irons-Treharne argument per quadrature point (the nonzero spectrum of
 *   M_e^-1 G_q^T A_q G_q is that of T_q; lambda_max of a sum is at most the sum of the lambda_max; the Dirichlet mask only
 *   removes rows and columns).  At order 1 and u = 0 it is the quantity of saa_operator_element_bound, reached another way.
 *   It is a BOUND, typically 1.4 to 2.3 times omega_max on well-shaped meshes and more on slivers: 2/max_e omega_e is a
 *   certified step, not a sharp one.
 *   omega_e_dev: n_elems device doubles, or NULL.  *omega_max, *argmax: the maximum and its element, ties to the lowest
 *   index, by a two-stage reduction in a fixed order (no floating-point atomics: bitwise repeatable); 0 and -1 when no
 *   element enters the maximum.  counts (3 host words, or NULL): [0] elements with detJ <= 0 at a point - the bound is
 *   certified only when this is 0; [1] elements with !(J > 0) at a point under neo-Hooke, NaN included: their omega_e is 0 and
 *   they leave the maximum, as the force pass drops them; [2] elements whose omega_e is not finite: the stored value stays as
 *   computed, they are left out of the maximum and counted, never dropped silently.
 *   An order-2 call uses the element contributions scratch for the mass shares.  Synchronises the stream, like
 *   saa_operator_element_bound.  SAA_E_ARG, before the handle or the device is looked at: a material outside {0, 1, 2}; then a
 *   null handle, null omega_max or argmax, null u_dev with a nonlinear material.
 * saa_operator_stepper_set_dt: an exact change of the step.  With v- = (d0 - dn)/dt_old, h = (dt_old + dt_new)/2 and
 *   a = (scale f - s)/m, s = f_int(d0) of the stepper's current material and scale the ramp factor at the current tn (the one
 *   the next step will use), the variable-step central-difference scheme is
 *     m (v+ - v-)/h + alpha m (v+ + v-)/2 + s = scale f,   d1 = d0 + dt_new v+ ,
 *   and the unchanged constant-step update of saa_operator_stepper_step with dt_new gives that same d1 when dn is replaced by
 *   dn' = d0 - dt_new v',
 *     v+ = ((1/h - alpha/2) v- + a) / (1/h + alpha/2),   v' = ((1/dt_new + alpha/2) v+ - a) / (1/dt_new - alpha/2).
 *   The call runs the stepper's own element pass at d0 into the contributions scratch (the pass set_material selected, the
 *   linear one included), one node pass that sums a node's contributions in ascending element order and overwrites dn with
 *   dn' (0 on Dirichlet dofs and at nodes without elements), and stores dt_new.  tn, the step index, the recorder and the
 *   stepper's inversion counters are left alone: the element pass of this call counts into the handle's scratch counter.
 *   dt_new == dt launches nothing and leaves the state bit-equal.  Enqueued: no host synchronisation.
 *   SAA_E_ARG: a null handle; dt_new not finite or <= 0; alpha > 0 and dt_new >= 2/alpha.  SAA_E_STATE: between step_begin and
 *   step_finish; with a shared set (a rank holds only its share of s); while the energy balance is on (its identity assumes
 *   one dt); with the "passes" option not at 3.
 *   WHICH dt to set is the caller's policy.  2/max_e omega_e of saa_operator_tangent_bound is certified and pessimistic;
 *   scaling the Lanczos step of the linear operator by min(1, bound(0)/bound(d)) (OperatorStepper.follow_time_step,
 *   "anchored") follows the stiffening without the pessimism but is a HEURISTIC, not a certificate.
 */
int saa_operator_tangent_bound(saa_operator *op, int32_t material, const double *u_dev /* NULL allowed with LINEAR */,
                               double *omega_e_dev /* n_elems, or NULL */, double *omega_max, int32_t *argmax,
                               int64_t *counts /* host, 3 words, or NULL */);
int saa_operator_stepper_set_dt(saa_operator_stepper *st, double dt_new);

/*
 * Implicit dynamics on the operator handle (csrc/saa_opimp.hip): an unconditionally stable time integrator next to the explicit
 * stepper above, either element order, all three materials.  Newmark with beta = 1/4, gamma = 1/2 (the trapezoidal rule) on the
 * system the explicit stepper integrates, with the diagonal mass m the caller passes (saa_operator_lumped_mass: HRZ at order 2),
 * the un-ramped load f, scale(t) = ramp ? min(t, 1) : 1, and mass-proportional damping:
 *     m a + alpha m v + f_int(d) = scale(t) f   on free dofs;   d = v = a = 0 on Dirichlet dofs and at nodes without elements
 *     d1 = x,   v1 = 2/dt (x - d) - v,   a1 = 4/dt^2 (x - d - dt v) - a
 *     r(x) = scale(t + dt) f - f_int(x) - m (a1(x) + alpha v1(x)),   J(x) = K_T(x) + s,   s = (4/dt^2 + 2 alpha/dt) m
 * A step: the predictor x = d + dt v; full Newton steps x += dx with J dx = r solved by Jacobi-PCG from 0, preconditioner
 * 1 / (diag K + s), diag K that of the linear operator (saa_operator_diagonal); the PCG runs to eta |r| with the forcing term of
 * the static Newton, eta = min(0.1, 0.9 (|r_k| / |r_k-1|)^2), 0.1 on a step's first iteration, floored at 0.1 tol scale / |r_k| so
 * that it never asks for more than the tolerance needs; it stops at the first p . J p <= 0 and hands back the iterate so far, or
 * the preconditioned residual if it has none.  With SAA_MATERIAL_LINEAR the one system is solved to tol.  A step has converged
 * when |r| <= tol max(|scale f|, |f_int(x)|, |m (a1 + alpha v1)|), 2-norms over the free dofs - the three terms of the balance,
 * so that a run at rest or at steady state has a meaningful scale.  NOT provided: a line search, an automatic cut of dt,
 * HHT-alpha, a consistent mass, partitions, an energy table.
 * The loops run on the device.  The element passes are those of saa_operator_apply, saa_operator_internal_force and
 * saa_operator_tangent_apply; the node passes, the PCG vector passes and the reductions are kernels of their own: block partials
 * and a fixed-order final sum folded into the kernel that needs it, 4 launches per PCG iteration, no floating-point atomics -
 * every result is bitwise repeatable and independent of how a run is split into calls.  The host reads one small status block
 * (iteration count, |r|, guard flag, inversion count) once per Newton iteration and every check_every PCG iterations, and once at
 * the end of the linear material's solve: that step is accepted on the recurrence residual of its PCG over the scale at the
 * solved x (one more residual pass gives it; the solve is repeated from there if the scale has fallen below what the
 * recurrence residual needs), because a residual evaluated afresh has the round-off floor of f_int (eps times the
 * cancellation inside it), which a tight tol lies below.
 *
 * saa_operator_shifted_apply: out = K_T(u) v + shift (.) v, 0 on Dirichlet dofs; u, v are masked on input as
 *   saa_operator_tangent_apply masks them, u_dev may be NULL with SAA_MATERIAL_LINEAR.  shift_dev: 3 * n_nodes device doubles, or
 *   NULL - then out is bit-equal to saa_operator_tangent_apply (same element pass, same sum order).  dot_dev: a device double that
 *   receives v . out over the free dofs, or NULL.  n_inverted (host, or NULL) as saa_operator_tangent_apply; reading it
 *   synchronises the stream.  SAA_E_ARG, before the device is touched: a material outside {0, 1, 2}, a null handle, v_dev or
 *   out_dev, null u_dev with a nonlinear material.
 * saa_operator_implicit_create: borrows the handle, which must outlive the stepper (and serves one stepper at a time: the
 *   contributions scratch is the handle's).  Copies mass and load (3 * n_nodes device doubles each); the state starts as
 *   _set_state(NULL, NULL, 0) leaves it: d = v = 0, t = 0, a = scale(0) f / m.  Synchronises once: SAA_E_ARG when the mass is not > 0 at a node that has elements; also for dt or alpha not
 *   finite, dt <= 0, alpha < 0, a material outside {0, 1, 2}, null pointers - those before the device is touched.
 * _set_state: d, v (NULL = zeros) are copied with the mask applied, a = (scale(t) f - f_int(d) - alpha m v) / m.  Enqueued.
 * _get_state: any output may be NULL; synchronises.
 * _set_recorder: layout and rule of saa_operator_stepper_set_recorder - row-major (3 * n_nodes, n_cols), the d of step index i
 *   goes to column i / save_every when i % save_every == 0 and the column exists; NULL switches it off.
 * _set_option: "tol" (1e-10), "max_newton" (25), "max_cg" (20 * 3 * n_nodes, per solve), "check_every" (25).  SAA_E_ARG: unknown
 *   name, tol outside (0, 1), a count that is not a whole number >= 1.
 * _set_dt: stores dt and recomputes s and the preconditioner; the scheme is one-step, so the state needs no surgery.
 * _step: up to nsteps steps.  A step is NOT accepted when max_newton Newton iterations did not converge it (reason 1), a
 *   residual is not finite (2), or - neo-Hooke - a trial x has an inverted element, by the counter words of the force pass (3).
 *   Then d, v, a, t and the step index stay those of the last accepted step, bit for bit, and the call returns SAA_OK with
 *   converged = 0, the reason and the number of steps done.  newton_iterations and cg_iterations are totals of the call;
 *   residual is the last |r| over its scale.  nsteps == 0 does nothing.  SAA_E_ARG: null handle or info, nsteps < 0.
 */
int saa_operator_shifted_apply(saa_operator *op, int32_t material, const double *u_dev /* NULL allowed with LINEAR */,
                               const double *v_dev, const double *shift_dev /* or NULL */, double *out_dev,
                               double *dot_dev /* device double, or NULL */, int64_t *n_inverted /* host, or NULL */);
typedef struct saa_operator_implicit saa_operator_implicit;
typedef struct saa_implicit_info {
  int32_t steps_done;         /* accepted steps of this call */
  int32_t converged;          /* 1: every requested step was accepted */
  int32_t reason;             /* 0 ok, 1 max_newton reached, 2 residual not finite, 3 inverted element (neo-Hooke) */
  int32_t reserved;
  int64_t newton_iterations;  /* of this call */
  int64_t cg_iterations;      /* of this call */
  double residual;            /* the last |r| / max(|scale f|, |f_int|, |m (a1 + alpha v1)|) */
} saa_implicit_info;
int saa_operator_implicit_create(saa_operator *op, const double *mass_dev, const double *f_ext_dev, double dt, double alpha,
                                 int32_t ramp, int32_t material, saa_operator_implicit **out);
int saa_operator_implicit_set_state(saa_operator_implicit *st, const double *d_dev, const double *v_dev, double t);
int saa_operator_implicit_get_state(saa_operator_implicit *st, double *d_dev, double *v_dev, double *a_dev, double *t);
int saa_operator_implicit_set_recorder(saa_operator_implicit *st, double *traj_dev, int64_t n_cols, int32_t save_every,
                                       int64_t next_step_index);
int saa_operator_implicit_set_option(saa_operator_implicit *st, const char *name, double value);
int saa_operator_implicit_set_dt(saa_operator_implicit *st, double dt);
int saa_operator_implicit_step(saa_operator_implicit *st, int32_t nsteps, saa_implicit_info *info);
int saa_operator_implicit_destroy(saa_operator_implicit *st);

/*
 * Finite-strain stress recovery (csrc/saa_stress_fs.hip): what saa_operator_stress / saa_operator_stress_p2 are to the linear
 * material, for the two materials above on a handle of either order.  At each point of the K rule (nq = 1 on an order-1
 * handle, the four Gauss points on an order-2 handle) H = grad_X x, formed as the force pass of that order forms it; x is read
 * as given: the Dirichlet mask is NOT applied, as in the linear stress entries.  With F = I + H, A = cof(H):
 *     J - 1 = tr H + tr A + det H,   det_f = 1 + (J - 1),   ln J = log1p(J - 1),
 *     G = F^-T - I = (A - H^T - (tr A + det H) I) / J   (never from an inverse of I + H)
 *   SAA_MATERIAL_SVK          E = (H + H^T + H^T H)/2,  S = lambda tr(E) I + 2 mu E,  sigma = F S F^T / J,
 *                             W = lambda/2 tr(E)^2 + mu E:E
 *   SAA_MATERIAL_NEO_HOOKEAN  S = -mu (G + G^T + G^T G) + lambda ln J (I + G + G^T + G^T G),
 *                             sigma = (mu (H + H^T + H H^T) + lambda ln J I) / J,
 *                             W = mu/2 (F:F - 3) - mu ln J + lambda/2 (ln J)^2, evaluated as saa_operator_internal_force does
 * measure = SAA_STRESS_PK2 writes S (second Piola-Kirchhoff, reference configuration), SAA_STRESS_CAUCHY sigma; F S = P of
 * saa_operator_internal_force and P F^T / J = sigma.  Both vanish under a rigid motion to the rounding of x.  von_mises is
 * sqrt(((s_xx - s_yy)^2 + (s_yy - s_zz)^2 + (s_zz - s_xx)^2)/2 + 3 (s_yz^2 + s_xz^2 + s_xy^2)) of the chosen measure.  The
 * three differences are formed before the pressure that the normal stresses share is added, for every material and measure
 * (for the Cauchy stress of SVK from (2 mu F E F^T + lambda tr(E) (H + H^T + H H^T)) / J), so that von_mises keeps its
 * digits where lambda is many times mu and the stress nearly hydrostatic.
 * energy[e] = sum_q w_q |detJ_q| W(F_q), the stored energy of the element (that of saa_operator_internal_force).
 *
 * Layouts are those of the linear entries, so that saa_operator_nodal_average / saa_operator_stress_error (order 1) and
 * saa_operator_nodal_stress_p2 / saa_operator_stress_error_p2 (order 2) take the fields unchanged: Voigt rows xx, yy, zz, yz,
 * xz, xy (no factor on the shear rows: these are stresses); m = 1..16 column-major columns;
 *   order 1: stress[column][6 e + c],          von_mises, det_f[column][e],        energy[column][e]
 *   order 2: stress[column][24 e + 6 q + c],   von_mises, det_f[column][4 e + q],  energy[column][e]
 * energy_total, von_mises_max and von_mises_argmax (a point index nq e + q, the lowest on ties; -1 and 0.0 when no point
 * holds a value) have m entries.  Any output may be NULL; with every output NULL nothing is launched.
 *
 * Inversion.  An element with !(J > 0) at any of its points (NaN included) is inverted for a column under neo-Hooke with
 * either measure and under either material with the Cauchy measure; SVK with PK2 does not look at J.  An inverted element
 * writes 0 to stress, von_mises and energy of that column, is left out of the column's total and maximum, and is counted in
 * n_inverted[column] (host, m entries, or NULL).  Asking for the count synchronises the stream; otherwise the call is
 * enqueued on the handle's stream.  det_f always holds the computed value, so that the inverted points can be found.  One
 * column's inversion or NaN does not touch another column.  The per-column counters are device words updated with integer
 * atomics; there are no floating-point atomics, every output is bitwise repeatable and a column's results do not depend on
 * the other columns of the call.  An order-2 handle reads its reduced geometry table (made on first need, see above).
 *
 * SAA_E_ARG with the entry named in saa_last_error, before the handle or the device is looked at: a material outside {1, 2}
 * (the linear material has saa_operator_stress and saa_operator_stress_p2); a measure outside {0, 1}; then a null handle or a
 * null x_dev; m outside 1..16; a leading dimension below its minimum (3 * n_nodes, 6 * nq * n_elems, nq * n_elems, nq *
 * n_elems, n_elems) for a non-null output.
 */
#define SAA_STRESS_PK2 0
#define SAA_STRESS_CAUCHY 1
int saa_operator_stress_finite(saa_operator *op, int32_t material, int32_t measure, int32_t m,
                               const double *x_dev, int64_t ldx,
                               double *stress_dev, int64_t ld_stress,      /* 6*nq*n_elems per column */
                               double *von_mises_dev, int64_t ld_vm,       /* nq*n_elems per column  */
                               double *det_f_dev, int64_t ld_det,          /* nq*n_elems per column  */
                               double *energy_dev, int64_t ld_elem,        /* n_elems per column     */
                               double *energy_total_dev, double *von_mises_max_dev, int32_t *von_mises_argmax_dev,
                               int64_t *n_inverted /* host, m entries, or NULL */);

/*
 * Shared-node predictor: the per-rank LSTM encoder-decoder of Tools/DNN_tools.py:16-98 (2-layer bidirectional encoder of
 * width hidden_size, decoder LSTM of width 2*hidden_size + Linear) evaluated for all filter_size phase offsets of one
 * prediction window - what Tools/DNN_prediction.py:38-55 (`encoder_decoder_predictor`) computes with filter_size
 * sequential batch-1 passes on the CPU - as four launches (two f32 matrix-core GEMMs for the input projections, one
 * recurrence kernel, one output GEMM that scales back and writes the table).
 *
 * saa_predictor_create replaces `call_model` (DNN_prediction.py:18-34): `weights` are host pointers to the 22 fp32
 * tensors of the reference's state_dict in ITS order (Model_training.py:179-180 saves them):
 *   encoder.lstm_encoder.{weight_ih, weight_hh, bias_ih, bias_hh}_l0, the same four _l0_reverse, _l1, _l1_reverse,
 *   decoder.lstm_decoder.{weight_ih, weight_hh, bias_ih, bias_hh}_l0, decoder.fc.weight, decoder.fc.bias
 * (row-major, PyTorch's gate order i, f, g, o).  They are copied; the caller may free them after the call.
 * filter_size >= 2, hidden_size <= 128.
 */
typedef struct saa_predictor saa_predictor;
int saa_predictor_create(int32_t device, int32_t input_size, int32_t hidden_size, int32_t n_past, int32_t n_future,
                         int32_t filter_size, const float *const *weights, int32_t n_weights, saa_predictor **out);

/* `encoder_decoder_predictor(device, n, model, n_p, n_f, n_s, input_size, d_sol, scale_max, scale_min)`
 * (DNN_prediction.py:38-55) on device buffers: reads rows [n - n_past*filter_size, n) of the fp64 history `hist_dev`
 * (hist_rows x input_size, row stride ld_hist doubles: d_sol of Online_predictor.py:260,301), scales them to [-1, 0]
 * (DNN_tools.py:272-275), runs the model in fp32 and writes the (filter_size*n_future) x input_size fp64 table (row stride
 * ld_table) whose row k is the prediction for step n + k (`NF`, DNN_prediction.py:45,53-54; what saa_step_predicted
 * consumes).  Enqueued on `stream` (a hipStream_t; null = the null stream); returns without synchronising. */
int saa_predictor_predict(saa_predictor *p, const double *hist_dev, int64_t hist_rows, int64_t ld_hist, int64_t n,
                          double scale_max, double scale_min, double *table_dev, int64_t ld_table, void *stream);

int saa_predictor_destroy(saa_predictor *p);

/* The pointwise part of one LSTM step and its backward pass, for the training loop (`model_train`, DNN_tools.py:103-165,
 * whose decoder steps are `torch.nn.LSTM` calls, DNN_tools.py:73-79): device pointers, fp32, `gates` = (batch, 4*width)
 * pre-activations in PyTorch's order i, f, g, o;  c = f c_prev + i g,  h = o tanh(c).  The forward keeps the activated gates
 * (`act`, batch x 4*width) and tanh(c) for the backward, which turns the gradients with respect to h and c (either may be
 * null = zero) into those with respect to the pre-activations and c_prev.  Enqueued on `stream`; capturable in a HIP graph. */
int saa_lstm_cell_forward(int32_t device, int32_t batch, int32_t width, const float *gates_dev, const float *c_prev_dev,
                          float *h_dev, float *c_dev, float *act_dev, float *tanh_c_dev, void *stream);
int saa_lstm_cell_backward(int32_t device, int32_t batch, int32_t width, const float *act_dev, const float *tanh_c_dev,
                           const float *c_prev_dev, const float *dh_dev, const float *dc_next_dev, float *dgates_dev,
                           float *dc_prev_dev, void *stream);

/* A whole LSTM recurrence of the training pass in one launch, and its backward pass in one launch (`model_train`,
 * DNN_tools.py:103-165: encoder `nn.LSTM`, DNN_tools.py:32, and the decoder steps, :73-79; widths 50 = the encoder's hidden
 * size and 100 = the decoder's, Model_training.py:36-40 - other widths are refused and stay with PyTorch):
 *   gates_t = pre[b, t, :] + h_{t-1} W^T,  c_t = f c_{t-1} + i g,  h_t = o tanh(c_t)   over t = 0..steps-1 (reverse: downwards),
 * `pre_dev` (batch, steps, 4*width) = input projections + biases, `w_dev` (4*width, width) row-major, `h0_dev` / `c0_dev`
 * (batch, width) or null = zero.  The forward writes every h_t (`h_all_dev`, batch x steps x width; the last state is its
 * last processed row) and keeps c_t, the activated gates and tanh(c_t) for the backward, which turns the gradients with
 * respect to every h_t (`dh_all_dev`) and the final c (`dc_last_dev`, may be null) into those with respect to `pre`, h0 and
 * c0.  The weight gradient is one product outside: dW = dpre^T . h_prev over all rows and steps. */
int saa_lstm_recurrence_forward(int32_t device, int32_t batch, int32_t steps, int32_t width, int32_t reverse, const float *pre_dev,
                                const float *h0_dev, const float *c0_dev, const float *w_dev, float *h_all_dev, float *c_all_dev,
                                float *act_dev, float *tanh_c_dev, void *stream);
int saa_lstm_recurrence_backward(int32_t device, int32_t batch, int32_t steps, int32_t width, int32_t reverse,
                                 const float *dh_all_dev, const float *dc_last_dev, const float *c0_dev, const float *w_dev,
                                 const float *c_all_dev, const float *act_dev, const float *tanh_c_dev, float *dpre_dev,
                                 float *dh0_dev, float *dc0_dev, void *stream);

/* The three figures `model_train` / `model_test` accumulate per batch (DNN_tools.py:144-155,196-205) - the mean square error
 * of `out_dev` against `target_dev` (n fp32 elements each), 1 - mse / mean((y - mean y)^2) and 1 - mse / mean(y^2) - added to
 * the three doubles `sums3_dev`; sums in fp64.  `scratch3_dev`: three doubles, zero before the first call, left zero. */
int saa_train_stats(int32_t device, int64_t n, const float *out_dev, const float *target_dev, double *scratch3_dev,
                    double *sums3_dev, void *stream);

/* Timing aid for bench.py: runs `nsteps` saa_step steps bracketed by HIP events recorded on the
 * handle's stream and returns the elapsed milliseconds (kernel time incl. launch gaps). */
int saa_time_steps(saa_solver *s, int32_t nsteps, double *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* SAA_HIP_H */
