/*
 * pisa_hip.h -- C ABI of libpisa_hip.so, the MI355X (gfx950) implementation of
 * PISA's per-event hot path:  prob3 oscillation -> flux x osc x aeff reweight
 * -> weighted N-D histogram -> LLH / chi2.
 *
 * Conventions
 *   - every entry point returns an int status: 0 = OK, negative = error
 *     (pisa_hip_strerror() gives the text).  No exceptions cross the ABI.
 *   - `d_` pointers are DEVICE pointers (hipMalloc'ed or torch-allocated
 *     tensor.data_ptr()); `h_` pointers are host pointers.  Small parameter
 *     blocks are passed by host pointer and travel in the kernel-argument
 *     segment.
 *   - `stream` is a hipStream_t cast to void* (NULL = default stream).  All
 *     calls are asynchronous w.r.t. the host unless the name ends in _host.
 *   - fp64 throughout (PISA FTYPE=float64); complex numbers are interleaved
 *     (re, im) doubles, matrices are row-major 3x3 -- i.e. exactly the memory
 *     layout of the numpy arrays the reference passes to its numba kernels.
 *   - the library is stateless apart from an optional scratch context.
 *
 * Each declaration names the reference interface it replaces (file:line
 * relative to the icecube/pisa tree).
 */
#ifndef PISA_HIP_H
#define PISA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PISA_HIP_OK 0
#define PISA_HIP_ERR_INVALID -1     /* bad argument (shape, NULL, range)            */
#define PISA_HIP_ERR_LAYERS -2      /* >120 layers (numba_osc_kernels.py:227)       */
#define PISA_HIP_ERR_HIP -3         /* HIP runtime error (see pisa_hip_last_hip_error) */
#define PISA_HIP_ERR_GEOMETRY -4    /* Earth model/detector geometry unsupported    */
#define PISA_HIP_ERR_NEGATIVE -5    /* negative counts passed to a metric (stats.py:231-240) */
#define PISA_HIP_ERR_OVERFLOW -6    /* weight outside the fixed-point accumulator range */
#define PISA_HIP_ERR_NOMEM -7

#define PISA_HIP_MAX_LAYERS 120     /* numba_osc_kernels.py:227 */
#define PISA_HIP_MAX_SHELLS 64      /* PREM-59 + atmosphere = 61 */
#define PISA_HIP_MAX_DIMS 3         /* translation.py:252 "can only do up to 3D" */
#define PISA_HIP_ACC_LIMBS 6        /* 6 x 32-bit payload limbs, see DESIGN.md */
#define PISA_HIP_MAX_POINTS 16      /* parameter points per multi-point call */

const char *pisa_hip_strerror(int status);
const char *pisa_hip_last_hip_error(void);
int pisa_hip_version(void);
/* number of visible GPUs (<=0: none). Does not initialise a device context. */
int pisa_hip_device_count(void);

/* ------------------------------------------------------------------ prob3 */

/* The scalar arguments of `propagate_array`
 * (pisa/stages/osc/prob3numba/numba_osc_hostfuncs.py:56-70), as prepared by
 * prob3.compute_function / calc_probs (pisa/stages/osc/prob3.py:429-450, 539-578). */
typedef struct {
    double dm[9];         /* dm_matrix  f8[3,3]   (osc_params.py:265-292)        */
    double mix[18];       /* PMNS       c16[3,3]  (osc_params.py:174-211)        */
    double mat_pot[18];   /* generalised matter potential c16[3,3] (prob3.py:539-557) */
    double mat_decay[18]; /* decay matrix c16[3,3] (prob3.py:559-563)            */
    double lri_pot[9];    /* LRI potential f8[3,3] (prob3.py:565-578)            */
    int64_t decay_flag;   /* +1 decay on, -1 off  (prob3.py:226-229)             */
} pisa_hip_prob3_params;

/* Replaces the gufunc `propagate_array` for one container
 * (numba_osc_hostfuncs.py:56-70 -> osc_probs_layers_kernel,
 * numba_osc_kernels.py:121-345).
 *   d_energy[n]; d_densities / d_distances: [n][n_layers] if
 *   layers_per_element != 0, else one shared row [n_layers];
 *   d_probability[n][3][3] (P[init][final]).
 * nubar = +1 / -1 (container aux datum). */
int pisa_hip_propagate_array(const pisa_hip_prob3_params *h_params, int64_t nubar,
                             const double *d_energy, const double *d_densities,
                             const double *d_distances, int64_t n, int32_t n_layers,
                             int32_t layers_per_element, double *d_probability, void *stream);

/* Same contract with HOST buffers (numpy arrays): allocates, copies, runs,
 * copies back, synchronises.  This is the call a reference-side binding would
 * use in place of the numba gufunc. */
int pisa_hip_propagate_array_host(const pisa_hip_prob3_params *h_params, int64_t nubar,
                                  const double *h_energy, const double *h_densities,
                                  const double *h_distances, int64_t n, int32_t n_layers,
                                  int32_t layers_per_element, double *h_probability);

/* Grid fast path used when calc_mode is a 2-D (true_energy x true_coszen)
 * binning (prob3.py:452-459 links the 12 containers into 'nu' and 'nubar'):
 * one launch evaluates nu AND nubar on every node.
 *   d_energy[n_e]       node energies along the energy axis
 *   d_densities/d_distances[n_cz][n_layers]   one row per coszen node
 *   node index = e_major ? iE*n_cz + jcz : jcz*n_e + iE   (container.py:769-773)
 *   d_prob_nu / d_prob_nubar [n_e*n_cz][3][3]  (either may be NULL)
 *   d_pepmu [2][3][n_e*n_cz][2] (may be NULL): compact gather tables
 *       pepmu[side][flav][node] = (P[e->flav], P[mu->flav]), side 0 nu / 1 nubar,
 *       i.e. prob_e / prob_mu of `fill_probs` (prob3.py:593-608) for every
 *       container class, laid out for one 16-byte gather per event. */
int pisa_hip_prob3_grid(const pisa_hip_prob3_params *h_params, const double *d_energy,
                        int32_t n_e, const double *d_densities, const double *d_distances,
                        int32_t n_cz, int32_t n_layers, int32_t e_major, double *d_prob_nu,
                        double *d_prob_nubar, double *d_pepmu, void *stream);

/* Planned form of the same computation.  A plan is built once per set of
 * layer rows (i.e. at setup, and again only when Ye / tomography parameters
 * change, prob3.py:461-475): it resolves the reference's layer-matrix cache
 * (numba_osc_kernels.py:230-249) per coszen row, gives mirrored layers of a row one
 * matrix and lists the distinct shell densities.  Per evaluation H(E, rho) is then
 * diagonalised per (energy, distinct density) instead of per node and layer, and
 * each row's chain is multiplied in parts.  Results equal pisa_hip_prob3_grid to
 * rounding, not bit for bit: <= 3e-13 absolute on the grid of tests/golden/prob3_grid_prem12.npz
 * (tests/test_gpu_kernels.py), and both within 1e-11 of the exact probabilities from 0.1 GeV to
 * 100 TeV (tests/test_gpu_prob3_exact.py: 9.3e-12 this form's worst, 8.3e-12 the planned one's).
 * plan_create synchronises (it reads the rows back); the planned call is async. */
typedef struct pisa_hip_grid_plan pisa_hip_grid_plan;
int pisa_hip_grid_plan_create(const double *d_densities, const double *d_distances, int32_t n_cz,
                              int32_t n_layers, pisa_hip_grid_plan **out);
int pisa_hip_grid_plan_destroy(pisa_hip_grid_plan *plan);
int pisa_hip_prob3_grid_planned(const pisa_hip_prob3_params *h_params, pisa_hip_grid_plan *plan,
                                const double *d_energy, int32_t n_e, int32_t e_major,
                                double *d_prob_nu, double *d_prob_nubar, double *d_pepmu,
                                void *stream);

/* Production-height averaging.  Semantics of `prop_height_range` of the reference's nuSQuIDS stage
 * (pisa/stages/osc/nusquids.py:83-88, 573-606): the production height is uniform in [mean - range/2, mean + range/2],
 * projected onto the neutrino's direction, i.e. uniform in path length between the lengths L_min and L_max that
 * the two heights give.  Here the first traversed layer of a row (the atmosphere, electron density exactly 0)
 * has the length Lbar = (L_min + L_max) / 2 and `avg_range` holds dL = L_max - L_min per row; the probabilities are
 * the mean over that layer's length in [Lbar - dL/2, Lbar + dL/2], in closed form ("Production-height
 * average": with W = U.T, D_j = W[b][j] conj(U[a][j]), x_jk = (dm_j0 - dm_k0) 2.534 (dL/E) / 2,
 * P_avg[a->b] = sum_j |D_j|^2 + 2 sum_{j<k} sin(x_jk)/x_jk Re(D_j conj(D_k))).  A row or element with range 0 gets the
 * bits of the plain call.  PISA_HIP_ERR_INVALID, before anything is launched that writes an output: a negative
 * or non-finite range; a positive range on a row whose first traversed layer has a density != 0; a positive range
 * together with decay_flag == 1 or a non-zero lri_pot (the first layer is then not diagonal in the mass basis).
 *
 * Planned form: h_avg_range[n_cz] in km (NULL clears it: the plan then launches exactly the kernels of a plan that
 * never had one).  The range stays with the plan and serves pisa_hip_prob3_grid_planned, _planned_multi and the
 * evaluator.  Synchronises the device. */
int pisa_hip_grid_plan_set_avg_range(pisa_hip_grid_plan *plan, const double *h_avg_range);

/* Reference-order array form: the contracts of pisa_hip_propagate_array / _host plus d_avg_range: [n] if
 * layers_per_element != 0, else [1] for the shared row; NULL is the plain call.  The device form checks ranges and
 * rows with a small kernel and waits for its verdict before it launches the propagation (one stream
 * synchronisation per call). */
int pisa_hip_propagate_array_avg(const pisa_hip_prob3_params *h_params, int64_t nubar,
                                 const double *d_energy, const double *d_densities,
                                 const double *d_distances, const double *d_avg_range, int64_t n,
                                 int32_t n_layers, int32_t layers_per_element, double *d_probability,
                                 void *stream);
int pisa_hip_propagate_array_avg_host(const pisa_hip_prob3_params *h_params, int64_t nubar,
                                      const double *h_energy, const double *h_densities,
                                      const double *h_distances, const double *h_avg_range, int64_t n,
                                      int32_t n_layers, int32_t layers_per_element,
                                      double *h_probability);

/* Earth model as held by `Layers` (pisa/stages/osc/layers.py:216-335, 411-439):
 * shells ordered from the production sphere inwards. */
typedef struct {
    int32_t n_shell;
    double r_detector;
    double radii[PISA_HIP_MAX_SHELLS];
    double rhos[PISA_HIP_MAX_SHELLS];         /* electron-fraction weighted */
    double coszen_limit[PISA_HIP_MAX_SHELLS]; /* layers.py:308-335 */
} pisa_hip_earth;

/* Replaces `extCalcLayers` (layers.py:38-169).  Outputs [n][max_layers],
 * zero padded; max_layers >= 2*n_shell (layers.py:244).  d_n_layers may be
 * NULL.  d_status (int32, may be NULL) is set non-zero if any coszen hit the
 * geometry the reference cannot handle (it raises a broadcast error there). */
int pisa_hip_calc_layers(const pisa_hip_earth *h_earth, const double *d_coszen, int64_t n,
                         int32_t max_layers, double *d_n_layers, double *d_densities,
                         double *d_distances, int32_t *d_status, void *stream);

/* Event-by-event prob3 (calc_mode = "events", prob3.py:406-409 + 581-588)
 * WITHOUT materialising densities/distances[n][L]: the layer path of every
 * event is rebuilt in-kernel from its coszen with the shell table in LDS. */
int pisa_hip_prob3_events(const pisa_hip_prob3_params *h_params, const pisa_hip_earth *h_earth,
                          int64_t nubar, const double *d_energy, const double *d_coszen,
                          int64_t n, double *d_probability, int32_t *d_status, void *stream);

/* The same for several containers in ONE launch (prob3.py:581-588 loops over the
 * 12 containers), optionally writing only the two probabilities the container
 * needs: d_pepmu[n][2] = (P[e->flav], P[mu->flav]) = (prob_e, prob_mu) of
 * `fill_probs` (prob3.py:593-608). */
typedef struct {
    int64_t n_events;
    const double *d_energy;
    const double *d_coszen;
    double *d_probability;   /* [n][3][3] or NULL */
    double *d_pepmu;         /* [n][2] or NULL    */
    int32_t nubar;           /* +1 / -1 */
    int32_t flav;            /* 0, 1, 2 */
} pisa_hip_event_set;
int pisa_hip_prob3_events_multi(const pisa_hip_prob3_params *h_params,
                                const pisa_hip_earth *h_earth, const pisa_hip_event_set *h_sets,
                                int32_t n_sets, int32_t *d_status, void *stream);

/* `fill_probs` (numba_osc_hostfuncs.py:206-221): out[i] = P[i][init_flav][flav]. */
int pisa_hip_fill_probs(const double *d_probability, int64_t init_flav, int64_t flav, int64_t n,
                        double *d_out, void *stream);

/* ------------------------------------------------------------ translation */

typedef struct {
    int32_t ndim;                         /* 1..3 */
    int64_t nbins[PISA_HIP_MAX_DIMS];
    double mins[PISA_HIP_MAX_DIMS];       /* regularised (linear) domain:      */
    double maxs[PISA_HIP_MAX_DIMS];       /* ln(lo), ln(hi) for log dimensions */
} pisa_hip_binning;

/* `lookup_regular_{1,2,3}d` and `_array` variants
 * (pisa/core/translation.py:417-501): nearest-bin gather, 0 outside
 * [min,max).  d_flat_hist[n_bins][width], d_out[n][width]. */
int pisa_hip_lookup_regular(const pisa_hip_binning *h_binning, const double *const *h_d_sample,
                            int64_t n, const double *d_flat_hist, int32_t width, double *d_out,
                            void *stream);

/* `histogram(sample, weights, binning, averaged)` for regular linear
 * binnings (translation.py:90-129, 171-205 -> fast_histogram.histogramdd).
 * d_weights may be NULL (counts).  Sums are accumulated in 192-bit fixed
 * point (order independent, bit-reproducible) and rounded once to fp64.
 * averaged != 0 divides by the per-bin count with NaN->0 (translation.py:118-127). */
int pisa_hip_histogram_regular(const pisa_hip_binning *h_binning,
                               const double *const *h_d_sample, int64_t n,
                               const double *d_weights, int32_t averaged, double *d_hist,
                               void *stream);

/* ------------------------------------- fused reweight + histogram (hot loop) */

/* Digitise event coordinates once: d_index[i] = flat C-order bin of the regular
 * binning, or -1 outside [min,max) / NaN (same rule as the lookups and
 * histograms above).  Event coordinates do not change between evaluations, so
 * the engine stores the calc-grid node and the output bin of every event as
 * int32 columns (the reference pre-digitises irregular dimensions the same way,
 * utils/hist.py:100-113). */
int pisa_hip_event_indices(const pisa_hip_binning *h_binning, const double *const *h_d_sample,
                           int64_t n, int32_t *d_index, void *stream);

/* One PISA container (pisa/core/container.py:451) as seen by the fused
 * kernel: device columns + the aux scalars the stages read.  Either the
 * coordinate columns (d_grid_*, d_sample) or the pre-digitised index columns
 * (d_node, d_bin) must be given; the indexed form moves 40 B/event, the
 * coordinate form 48 + 8*D B/event. */
typedef struct {
    int64_t n_events;
    const double *d_grid_x;          /* lookup coordinate on calc-grid dim 0 (ln E if log) */
    const double *d_grid_y;          /* lookup coordinate on calc-grid dim 1               */
    const double *d_nu_flux;         /* [n][2]  (nue, numu) flux  (barr_simple.py:100)     */
    const double *d_weighted_aeff;   /* [n]                                              */
    const double *d_initial_weights; /* [n]   (toy_event_generator.py:101-104)           */
    const double *d_sample[PISA_HIP_MAX_DIMS]; /* output-binning coordinates, regularised */
    const int32_t *d_node;           /* [n] calc-grid node of each event, -1 outside (optional) */
    const int32_t *d_bin;            /* [n] output bin of each event, -1 outside (optional)     */
    const int32_t *d_node_bin;       /* [n][2] the two above interleaved (optional, fastest)    */
    const double *d_aeff_w0;         /* [n][2] (weighted_aeff, initial_weights) interleaved (opt.) */
    const double *d_pepmu;           /* [n_nodes][2] this container's own (P_e, P_mu) table,
                                        overrides the grid tables (event-mode prob3: node = event) */
    int32_t flav;                    /* 0 e, 1 mu, 2 tau  (aux 'flav')                     */
    int32_t nubar;                   /* +1 / -1           (aux 'nubar')                    */
    double scale;                    /* aeff_scale*livetime_s*norms (aeff.py:78-86)        */
    const double *d_weighted_flux;   /* [n][2] optional COMPACT form, used together with d_node_bin:
                                        initial_weights*weighted_aeff*(nu_flux_e, nu_flux_mu), i.e. the
                                        factors of the weight that do not depend on the oscillation
                                        parameters multiplied once (24 B per event instead of 40).
                                        w = ((g_e*P_e) + (g_mu*P_mu)) * scale: the reference's product
                                        with the static factors associated first (differs from the
                                        40-B form by rounding, <= 3 ulp per weight).  The caller
                                        refreshes it when nu_flux changes (flux systematics). */
    /* 16-BIT INDEX form of the compact columns (20 B per event), for calc grids below 65535
     * nodes and output binnings below 65535 bins.
     * Given for every container it is the form used; it stands alone (d_node_bin and
     * d_weighted_flux may be NULL).  For a grid / binning it does not apply to these two
     * columns are ignored: the call uses the other forms if they are given as well and is
     * PISA_HIP_ERR_INVALID if not.  Both arrays are padded to a multiple of 256 events with events
     * outside the binning (index word 0xffffffff, flux pair 0). */
    const uint32_t *d_node_bin16;    /* [n_pad] node | bin << 16, 0xffff in a half = outside */
    const double *d_weighted_flux_q; /* [n_pad / 256][4][64][2]: d_weighted_flux with the pairs of a
                                        quad of consecutive events e = 4q + k stored at
                                        [q / 64][k][q % 64], so that the 64 lanes of a wavefront
                                        (one quad each) read 16 contiguous bytes per lane */
    /* PARTITIONED resident order (optional; 16-bit index form with an output binning beyond the LDS
     * accumulators, pisa_hip_hist_window_bins(n_bins) = W > 0): the caller has ordered the events so that
     * partition p = events [256 d_part_start[p], 256 d_part_start[p+1]) deposits only into bins
     * [p W, (p+1) W) (events outside the binning may sit anywhere), d_part_start[0] = 0,
     * d_part_start[n_part] = n_pad / 256.  The kernel then keeps every deposit in LDS and scans nothing.
     * Ignored (the general window path is used) unless part_width == W.  The histogram does not depend on
     * the order of the events: the same bits either way. */
    const int32_t *d_part_start;     /* DEVICE array [n_part + 1], units of 256 events, or NULL */
    int32_t n_part;
    int32_t part_width;
} pisa_hip_container;

/* 0 if the fused kernels keep all n_bins accumulators of a container in LDS, else the number of
 * consecutive bins W their LDS window holds (a multiple of 32). */
int pisa_hip_hist_window_bins(int64_t n_bins);
/* Workgroups the fused kernels give each container of a launch on the current device (a hint for a caller
 * that lays out the partitioned order: partitions that are whole numbers of a container's per-workgroup share
 * keep every workgroup inside one partition; any other layout is handled, only slower). */
int pisa_hip_hist_workgroups(const int64_t *h_n_events, int32_t n_containers, int32_t *h_workgroups);
/* The resident order of one container's events for the 16-bit index form (d_node_bin16 / d_weighted_flux_q): the
 * permutation that gathers the events that can deposit (d_node >= 0 and d_bin >= 0: the digitised calc-grid node and output
 * bin of every event, DEVICE int32[n]) into whole blocks of 256 -- sorted by node, dealt over the 32 LDS bank pairs inside
 * windows of 4 096, the blocks spread evenly among the blocks of events that deposit nothing.  No counterpart in the
 * reference (its events stay in file order; `container.py:981-1012` looks them up one by one): the sums are exact, so the
 * order is this build's to choose, and it is part of the set-up a caller pays once per event sample.
 * d_perm: DEVICE int64[n], out: position i of the resident order holds input event d_perm[i].  n_nodes: size of the calc
 * grid (d_node < n_nodes).  Asynchronous on `stream`; d_work: DEVICE scratch of pisa_hip_deposit_block_order_workspace(n)
 * bytes. */
int64_t pisa_hip_deposit_block_order_workspace(int64_t n);
int pisa_hip_deposit_block_order(const int32_t *d_node, const int32_t *d_bin, int64_t n, int64_t n_nodes,
                                 int64_t *d_perm, void *d_work, int64_t work_bytes, void *stream);
/* The resident order for a binning BEYOND the LDS accumulators (pisa_hip_hist_window_bins(n_bins) = W > 0): partition p holds
 * the events that deposit into bins [p W, (p + 1) W) -- sorted by node, whole 4 096-event windows of a partition of >= 8 192
 * events in the bank order --, topped up with idle events to whole blocks of 256 and interleaved with further idle blocks
 * (pisa_hip_container::d_part_start is the table the fused kernel then walks).  Two calls around the caller's block accounting:
 *   _sort      one key per event, one stable radix sort; h_counts[0 .. n_part) = depositing events of every partition,
 *              h_counts[n_part] = idle events (HOST, out; the call synchronises `stream`);
 *   _assemble  h_n_dep = those counts, h_dep_blocks[p] = ceil(h_n_dep[p] / 256), h_idle_blocks[p] = idle blocks partition p
 *              is interleaved with (depositing block q of its nb goes to block floor(q (nb + nf) / nb) of the partition):
 *              d_perm DEVICE int64[n], out, position i of the resident order holds input event d_perm[i]; whatever idle
 *              events the blocks do not use follow the last partition.  Synchronises `stream`.
 * Both take the SAME d_work (DEVICE, pisa_hip_partition_order_workspace(n) bytes: the sorted sequence lives in it between the
 * calls).  n_part <= 255, (n_part + 1) (n_nodes + 1) < 2^32.  No counterpart in the reference (its events stay in file
 * order): the sums are exact, so the order is this build's to choose. */
int64_t pisa_hip_partition_order_workspace(int64_t n);
int pisa_hip_partition_order_sort(const int32_t *d_node, const int32_t *d_bin, int64_t n, int64_t n_nodes, int32_t width,
                                  int32_t n_part, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream);
int pisa_hip_partition_order_assemble(const int32_t *d_bin, int64_t n, int32_t n_part, const int64_t *h_n_dep,
                                      const int64_t *h_dep_blocks, const int64_t *h_idle_blocks, int64_t *d_perm,
                                      void *d_work, int64_t work_bytes, void *stream);
/* The resident copies of one container's event columns in the order `d_perm` (the permutation above), in ONE launch: the
 * permuted columns themselves and the interleaved / folded forms the fused kernel reads -- what pisa_amd/engine.py built
 * with ~25 tensor operations per container (6 ms of a 24 ms set-up at 1e7 events, bound by their dispatch on the host).
 * out[k] = in[d_perm[k]] for every column; d_node_bin[k] = (node, bin); d_aeff_w0[k] = (aeff, w0); d_static_w[k] =
 * w0 * aeff; d_node_bin16[k] = node | bin << 16 with 0xFFFF for a negative index, 0xFFFFFFFF for n <= k < n_pad (n_pad = n
 * rounded up to whole blocks of 256 events).  All pointers DEVICE; columns double[n], d_nu_flux double[n][2], d_node /
 * d_bin int32[n], d_perm int64[n]; d_sample: up to three output-binning coordinate columns (n_sample of them).  No
 * counterpart in the reference (its containers keep file order, `container.py:933-1012`).  Asynchronous on `stream`. */
typedef struct {
    int64_t n, n_pad;
    const int64_t *d_perm;
    const double *d_grid_x, *d_grid_y, *d_nu_flux, *d_weighted_aeff, *d_initial_weights;
    const double *d_sample[3];
    const int32_t *d_node, *d_bin;
    double *o_grid_x, *o_grid_y, *o_nu_flux, *o_weighted_aeff, *o_initial_weights;
    double *o_sample[3];
    int32_t *o_node, *o_bin, *o_node_bin;
    double *o_aeff_w0, *o_static_w;
    int32_t *o_node_bin16;
    int32_t n_sample, reserved;
} pisa_hip_pack_set;
int pisa_hip_pack_resident_columns(const pisa_hip_pack_set *set, void *stream);

/* Fused  prob3.apply (prob3.py:621-622, with the grid->event lookup of
 * container.py:981-1012 / translation.py:427-438)  +  aeff.apply
 * (aeff.py:78-88)  +  hist.apply with error_method='sumw2'
 * (utils/hist.py:163-218)  over all containers in ONE pass over the events:
 *     w  = w0 * (f_e*P[e->flav] + f_mu*P[mu->flav]) * (aeff*scale)
 *     hist[c][bin] += w ;  sumw2[c][bin] += w*w
 * Result: d_limbs[n_containers][n_bins][2][PISA_HIP_ACC_LIMBS] int64 (zeroed by
 * the call) -- exact sums in 192-bit fixed point spread over six 32-bit-spaced
 * limbs, safe to SUM-all-reduce across ranks (integer addition is associative
 * => bit-reproducible for any workgroup schedule and any GPU count).
 * d_pepmu: gather tables of pisa_hip_prob3_grid (required for the indexed forms; the coordinate
 * form reads them too when they are given -- one 16-byte gather per event instead of two 8-byte ones
 * from the 72-byte records of d_prob_nu / d_prob_nubar, 25 % of that kernel -- and the full matrices
 * otherwise; both hold the same numbers).
 * d_status: int32 flag, set non-zero if a weight is not finite or >= 2^76. */
int pisa_hip_reweight_hist(const pisa_hip_container *h_containers, int32_t n_containers,
                           const pisa_hip_binning *h_calc_grid, const double *d_prob_nu,
                           const double *d_prob_nubar, const double *d_pepmu,
                           const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                           int32_t *d_status, void *stream);

/* Measurement hook: hipEvent_t handles (cast to void*, NULL to disable) that the
 * next pisa_hip_reweight_hist / pisa_hip_histogram_regular calls of this host
 * thread record immediately before and after the accumulate kernel on `stream`. */
int pisa_hip_profile_events(void *start_event, void *stop_event);

/* Unfused stage-by-stage variants (same arithmetic, one stage each) so that a
 * pipeline with other services interleaved still runs on the device. */
int pisa_hip_apply_osc_weights(const double *d_nu_flux, const double *d_prob_e,
                               const double *d_prob_mu, int64_t n, double *d_weights,
                               void *stream); /* prob3.py:621-622 */
/* the same with prob_e / prob_mu read at an element stride (columns of one table: the (P_e, P_mu) pairs of the
 * gather tables have stride 2) -- a stage that publishes such columns as views need not compact them */
int pisa_hip_apply_osc_weights_strided(const double *d_nu_flux, const double *d_prob_e,
                                       const double *d_prob_mu, int64_t prob_stride, int64_t n,
                                       double *d_weights, void *stream); /* prob3.py:621-622 */
int pisa_hip_apply_aeff(const double *d_weighted_aeff, double scale, int64_t n,
                        double *d_weights, void *stream); /* aeff.py:87 */

/* The whole weight chain of several containers in ONE launch (what the three stages' apply_functions do to
 * `weights` one after the other, on events or on the bins of a map):
 *   weights = copy(initial_weights)                   toy_event_generator.py:101-104 and the other loaders
 *   weights *= flux[:,0]*prob_e + flux[:,1]*prob_mu   prob3.py:621-622   (skipped if d_nu_flux == NULL)
 *   weights *= weighted_aeff * aeff_scale             aeff.py:87         (skipped if d_weighted_aeff == NULL)
 * with every step rounded to fp64 as the one-step calls above round it: the same bits as
 * copy -> pisa_hip_apply_osc_weights[_strided] -> pisa_hip_apply_aeff. */
typedef struct {
    int64_t n;
    const double *d_initial_weights; /* [n] */
    const double *d_nu_flux;         /* [n][2] or NULL */
    const double *d_prob_e;          /* read at element stride prob_stride */
    const double *d_prob_mu;
    int64_t prob_stride;
    const double *d_weighted_aeff;   /* [n] or NULL */
    double aeff_scale;
    double *d_weights;               /* [n] out */
} pisa_hip_chain_set;
int pisa_hip_weight_chain_multi(const pisa_hip_chain_set *h_sets, int32_t n_sets, void *stream);

/* Converts all-reduced limbs to fp64 maps: d_hist / d_sumw2 [n_containers][n_bins]
 * (either may be NULL). `errors` = sqrt(sumw2) is left to the caller (hist.py:215). */
int pisa_hip_hist_finalize(const int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                           double *d_hist, double *d_sumw2, int32_t *d_status, void *stream);

/* pisa_hip_reweight_hist without the initial clear of d_limbs: ADDS this call's
 * events to whatever the limbs hold (e.g. the zeros left behind by
 * pisa_hip_finalize_metric(clear_limbs=1), or the sums of another batch). */
int pisa_hip_reweight_hist_acc(const pisa_hip_container *h_containers, int32_t n_containers,
                               const pisa_hip_binning *h_calc_grid, const double *d_prob_nu,
                               const double *d_prob_nubar, const double *d_pepmu,
                               const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                               int32_t *d_status, void *stream);

/* ------------------------------------------------ the accumulate plan
 * Events outside the output binning deposit nothing at any parameter point, and which they are is fixed by the
 * binning and the events' static coordinates.  The resident order (pisa_hip_deposit_block_order) gathers the others
 * into whole blocks of 256 events; a plan lists, once per set of containers, the blocks that hold at least one event
 * whose BIN half of d_node_bin16 is not 0xffff (padding, 0xffffffff, is idle by the same rule; an event inside the
 * binning but outside the calc grid counts: it still forms its product and flags a non-finite flux).  A planned call
 * streams the listed blocks alone, dealt round robin to the wavefronts of the container's workgroups, and gives the
 * same limbs and the same status word as pisa_hip_reweight_hist[_acc]: the sums are exact in any order.
 *
 * _create   applies where pisa_hip_reweight_hist uses the 16-bit index form with every accumulator in LDS
 *           (d_node_bin16 / d_weighted_flux_q for every container with events, calc grid and binning below 65535
 *           entries, pisa_hip_hist_window_bins(n_bins) == 0).  Elsewhere it returns PISA_HIP_OK with *plan = NULL and
 *           the caller keeps to pisa_hip_reweight_hist[_acc].  Reads every index column once on `stream` and
 *           synchronises it (the block counts go to the host, where the work split is made: one workgroup per CU,
 *           dealt to the containers by their DEPOSITING events; a container without any gets none).
 * _destroy  NULL is fine.
 * _info     for tests and diagnostics: blocks of 256 events of one container, how many of them are listed, the
 *           workgroups it gets, and (h_dep_blocks != NULL: room for n_dep_blocks int32) the list itself, ascending.
 * _planned  pisa_hip_reweight_hist (clear_first != 0) or _acc (clear_first == 0) through the plan.  `scale` and every
 *           column pointer are read from h_containers at each call; the plan contributes the lists and the work
 *           split only.  PISA_HIP_ERR_INVALID if n_containers, an event count, the grid or the binning differ from
 *           what the plan was made from, or if the call would not use the 16-bit index form (no gather table).
 *
 * THE PLAN SNAPSHOTS WHICH BLOCKS DEPOSIT.  A caller that rewrites a d_node_bin16 column (another binning, another
 * event order, other events) makes a new plan.  Flux refreshes -- pisa_hip_fold_flux, the Barr folds -- write
 * d_weighted_flux_q only and leave a plan valid. */
typedef struct pisa_hip_hist_plan pisa_hip_hist_plan;
int pisa_hip_hist_plan_create(const pisa_hip_container *h_containers, int32_t n_containers,
                              const pisa_hip_binning *h_calc_grid, const pisa_hip_binning *h_out_binning,
                              pisa_hip_hist_plan **plan, void *stream);
int pisa_hip_hist_plan_destroy(pisa_hip_hist_plan *plan);
int pisa_hip_hist_plan_info(const pisa_hip_hist_plan *plan, int32_t container, int32_t *n_blocks,
                            int32_t *n_dep_blocks, int32_t *workgroups, int32_t *h_dep_blocks);
int pisa_hip_reweight_hist_planned(const pisa_hip_hist_plan *plan, const pisa_hip_container *h_containers,
                                   int32_t n_containers, const pisa_hip_binning *h_calc_grid,
                                   const double *d_prob_nu, const double *d_prob_nubar, const double *d_pepmu,
                                   const pisa_hip_binning *h_out_binning, int64_t *d_limbs, int32_t *d_status,
                                   int32_t clear_first, void *stream);

/* Largest n_containers*n_bins pisa_hip_finalize_metric accepts (one workgroup). */
#define PISA_HIP_FINALIZE_METRIC_MAX 4096

/* pisa_hip_hist_finalize + pisa_hip_metric(kind, d_actual, d_hist, d_sumw2,
 * n_maps = n_containers) in ONE launch, for the tail of a template evaluation
 * (hist.py:215 -> distribution_maker.py:274-281 -> map.py:1572-1604): same
 * arithmetic in the same order as the two separate calls, bit for bit.
 * d_hist / d_sumw2 [n_containers][n_bins] are written (required).
 * total[1] may be device memory or device-mapped pinned host memory (the host
 * then only waits for the stream; no copy kernel).
 * clear_limbs != 0: d_limbs is zero again when the kernel ends, ready for
 * pisa_hip_reweight_hist_acc.
 * d_status: overflow flag of the limbs (as pisa_hip_hist_finalize);
 * d_metric_status: PISA_HIP_ERR_NEGATIVE for negative inputs (as pisa_hip_metric).
 * PISA_HIP_ERR_INVALID if n_containers*n_bins > PISA_HIP_FINALIZE_METRIC_MAX. */
int pisa_hip_finalize_metric(int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                             double *d_hist, double *d_sumw2, int32_t kind,
                             const double *d_actual, double *total, int32_t *d_status,
                             int32_t *d_metric_status, int32_t clear_limbs, void *stream);

/* pisa_hip_finalize_metric for a template that is not just the sum of the histogrammed maps:
 * d_scale [n_containers][n_bins] (or NULL): per-bin factors of a stage that follows the histogram --
 *   discr_sys.hypersurfaces, `weights = clip(weights * s, 0, inf)`, `errors *= s`
 *   (hypersurfaces.py:251-259): the expectation of bin b is sum_c max(w_cb s_cb, 0), its variance
 *   sum_c sumw2_cb s_cb^2.  d_hist / d_sumw2 are written UNscaled.
 * d_extra [2][n_bins] (or NULL): expectation and variance of maps added to the template after the
 *   containers, in that order (the other pipelines of a DistributionMaker, distribution_maker.py:274-281). */
int pisa_hip_finalize_metric_scaled(int64_t *d_limbs, int32_t n_containers, int64_t n_bins,
                                    double *d_hist, double *d_sumw2, int32_t kind,
                                    const double *d_actual, const double *d_scale,
                                    const double *d_extra, double *total, int32_t *d_status,
                                    int32_t *d_metric_status, int32_t clear_limbs, void *stream);

/* ------------------------------------------------ several parameter points in one sweep
 * What a fit loop asks of the path: the minimiser settings of the reference are finite-difference
 * methods (settings/minimizer/l-bfgs-b_*.json, slsqp_*.json, driven from
 * pisa/analysis/analysis.py:2493-2670), i.e. n + 1 INDEPENDENT parameter points per gradient, and its
 * own timing protocol evaluates independent points as well
 * (pisa/scripts/benchmark_pipeline_performance.py:196-223).  The three calls below evaluate K points
 * where the reference -- and the single-point calls above -- would run K whole template evaluations
 * one after the other; per point the results are BIT-IDENTICAL to the single-point calls
 * (tests/test_gpu_multipoint.py). */

/* pisa_hip_prob3_grid_planned (osc.prob3 compute_function, prob3.py:581-608) for n_points parameter
 * blocks h_params[n_points] in one pair of launches.  Only the gather tables are written, the points
 * interleaved:  d_pepmu_points[2][3][n_e*n_cz][n_points][2]  (n_points == 1: the layout of d_pepmu).
 * All points must agree in decay_flag.  n_points <= PISA_HIP_MAX_POINTS. */
int pisa_hip_prob3_grid_planned_multi(const pisa_hip_prob3_params *h_params, int32_t n_points,
                                      pisa_hip_grid_plan *plan, const double *d_energy, int32_t n_e,
                                      int32_t e_major, double *d_pepmu_points, void *stream);

/* pisa_hip_reweight_hist (prob3.py:621-622 + aeff.py:78-88 + utils/hist.py:163-218) for n_points
 * parameter points in ONE pass over the event columns: the 20 B per event are read once, an event's
 * (P_e, P_mu) pairs of all points come from one contiguous run of d_pepmu_points (layout above) and
 * each point has its own accumulators.  Containers must carry the 16-bit index form (d_node_bin16,
 * d_weighted_flux_q) and use the shared grid tables (d_pepmu == NULL); PISA_HIP_ERR_INVALID otherwise
 * (the caller then evaluates point by point).
 * h_scales[n_points][n_containers] (or NULL = every point uses container.scale): aeff.py:78-86 scale
 * of each container at each point.
 * d_limbs[n_points][n_containers][n_bins][2][PISA_HIP_ACC_LIMBS]; clear_first != 0: zeroed by the
 * call, else the sums are ADDED to what they hold (the zeros pisa_hip_finalize_metric_multi leaves
 * behind with clear_limbs = 1, as pisa_hip_reweight_hist_acc).
 * A batch larger than pisa_hip_multi_points_per_pass(n_bins) is split into several sweeps. */
int pisa_hip_reweight_hist_multi(const pisa_hip_container *h_containers, int32_t n_containers,
                                 const pisa_hip_binning *h_calc_grid, const double *d_pepmu_points,
                                 int32_t n_points, const double *h_scales,
                                 const pisa_hip_binning *h_out_binning, int64_t *d_limbs,
                                 int32_t clear_first, int32_t *d_status, void *stream);
int pisa_hip_multi_points_per_pass(int64_t n_bins);

/* pisa_hip_finalize_metric_scaled for n_points sets of limbs, one workgroup per point:
 * d_limbs as pisa_hip_reweight_hist_multi leaves them, d_hist / d_sumw2 [n_points][n_containers][n_bins],
 * total[n_points] (device or device-mapped pinned host memory); d_actual and d_extra are shared by the
 * points, d_scale (may be NULL) is read at d_scale + point * scale_point_stride (0: shared). */
int pisa_hip_finalize_metric_multi(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                   int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                   const double *d_actual, const double *d_scale,
                                   int64_t scale_point_stride, const double *d_extra, double *total,
                                   int32_t *d_status, int32_t *d_metric_status, int32_t clear_limbs,
                                   void *stream);

/* pisa_hip_finalize_metric_multi with FOUR workgroups per point, for a caller that reads the value from
 * device-mapped pinned host memory in a fit loop (the conversions of the limbs are what the one-workgroup form
 * spends its time on).  Workgroup k takes the bins b = k (mod 4) of every container and leaves the sum of the
 * metric over its bins in partial[4 * point + k]; the caller adds
 *       total = (partial[0] + partial[2]) + (partial[1] + partial[3])
 * which is pisa_hip_finalize_metric_multi's value bit for bit (the same reduction tree, cut before its last two
 * levels).  Maps, limb clearing and status words as there; a negative input makes the partial of its workgroup NaN.
 * kind = PISA_HIP_METRIC_CHI2 is refused (stats.py:160-161: its all-bins-equal rule needs every bin). */
int pisa_hip_finalize_metric_split(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                   int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                   const double *d_actual, const double *d_scale,
                                   int64_t scale_point_stride, const double *d_extra, double *partial,
                                   int32_t *d_status, int32_t *d_metric_status, int32_t clear_limbs,
                                   void *stream);

/* pisa_hip_finalize_metric_split with n_parts = 4 or 16 workgroups per point: workgroup k takes the bins
 * b = k (mod n_parts) and leaves its sum in partial[n_parts * point + k]; the caller joins them along the
 * kernel's own reduction tree, cut n_parts wide:
 *      for (w = n_parts / 2; w >= 1; w /= 2) for (i = 0; i < w; i++) partial[i] += partial[i + w];   total = partial[0]
 * (n_parts = 4: (p0 + p2) + (p1 + p3)) -- pisa_hip_finalize_metric_multi's value bit for bit.  Sixteen workgroups
 * leave every thread at most one conversion of a limb sum: the tail of a 3 072-accumulator evaluation drops
 * from 6.4 to ~3.5 us. */
int pisa_hip_finalize_metric_parts(int64_t *d_limbs, int32_t n_points, int32_t n_containers,
                                   int64_t n_bins, double *d_hist, double *d_sumw2, int32_t kind,
                                   const double *d_actual, const double *d_scale,
                                   int64_t scale_point_stride, const double *d_extra, double *partial,
                                   int32_t n_parts, int32_t *d_status, int32_t *d_metric_status,
                                   int32_t clear_limbs, void *stream);

/* ------------------------------------------------ one template evaluation in ONE call
 * What `Pipeline.get_outputs()` followed by `Map.metric_total` amount to for the chain
 * osc.prob3 (calc grid) -> aeff.aeff -> utils.hist -> metric (pisa/core/pipeline.py:537-558 running
 * stage.py:584-586 per stage; the minimiser's callable pisa/analysis/analysis.py:2493-2670 calls exactly
 * that per point).  An evaluator is made once per pipeline from everything that does not change between
 * parameter points (the event columns, the binnings, the grid plan, the output buffers); per point
 *      pisa_hip_evaluator_eval(ev, params, kind, d_actual, ...)
 * enqueues  pisa_hip_prob3_grid_planned (gather tables only) -> pisa_hip_reweight_hist[_acc] (through a
 * pisa_hip_hist_plan of the evaluator's own, made by _create from the containers it copies, where one applies) ->
 * [all-reduce of the limbs] -> pisa_hip_finalize_metric_parts (16 workgroups, clear_limbs = 1)  -- the same
 * launches, the same bits as those four calls -- and, if asked to, waits for the value: the metric's sixteen
 * partial sums arrive in device-mapped pinned host memory and are joined as pisa_hip_finalize_metric_parts
 * documents.  A host binding crosses its FFI once per evaluation instead of three or four times.
 * kind = PISA_HIP_METRIC_CHI2 goes through the one-workgroup pisa_hip_finalize_metric.
 *
 * allreduce / comm (both NULL on one rank): the in-place int64 SUM of d_limbs over the ranks, called as
 *      allreduce(d_limbs, d_limbs, count, 4 (ncclInt64), 0 (ncclSum), comm, stream)
 * -- ncclAllReduce's own signature, so a binding passes RCCL's entry point and its communicator; the
 * library itself does not link RCCL. */
typedef struct pisa_hip_evaluator pisa_hip_evaluator;
typedef int (*pisa_hip_allreduce_fn)(const void *sendbuf, void *recvbuf, size_t count, int datatype,
                                     int op, void *comm, void *stream);
typedef struct {
    const pisa_hip_container *h_containers; /* copied */
    int32_t n_containers;
    int32_t n_e;                            /* energies of the calc grid */
    int32_t e_major;
    int32_t reserved;
    const pisa_hip_binning *h_calc_grid;    /* copied */
    const pisa_hip_binning *h_out_binning;  /* copied */
    pisa_hip_grid_plan *plan;               /* borrowed: must outlive the evaluator */
    const double *d_energy;                 /* [n_e] */
    double *d_pepmu;                        /* [2][3][nodes][2] gather tables (written per point) */
    int64_t *d_limbs;                       /* [n_containers][n_bins][2][PISA_HIP_ACC_LIMBS] */
    double *d_hist, *d_sumw2;               /* [n_containers][n_bins] (written per point) */
    double *partial;                        /* [16] device-mapped pinned host memory */
    int32_t *d_status, *d_metric_status;
    pisa_hip_allreduce_fn allreduce;
    void *comm;
} pisa_hip_evaluator_desc;
/* _create reads the d_node_bin16 columns of the containers (the evaluator's pisa_hip_hist_plan): it waits for the
 * whole device first, so columns written on any stream before the call are seen complete. */
int pisa_hip_evaluator_create(const pisa_hip_evaluator_desc *desc, pisa_hip_evaluator **out);
int pisa_hip_evaluator_destroy(pisa_hip_evaluator *ev);
/* aeff.py:78-86: the scale of one container (aeff_scale * livetime * norms) for the points to come */
int pisa_hip_evaluator_set_scale(pisa_hip_evaluator *ev, int32_t container, double scale);
/* limbs_zero != 0: d_limbs holds zeros (left by the previous evaluation's tail): no clearing pass.
 * wait_us > 0: poll `partial` for up to that many microseconds, then synchronise the stream; *value
 *   receives the metric.  wait_us == 0: enqueue only; the caller reads `partial` / synchronises itself.
 * On return with PISA_HIP_OK the limbs are zero again (after the stream has passed the tail). */
int pisa_hip_evaluator_eval(pisa_hip_evaluator *ev, const pisa_hip_prob3_params *h_params, int32_t kind,
                            const double *d_actual, int32_t limbs_zero, int64_t wait_us, double *value,
                            void *stream);

/* --------------------------------------------------------------------- KDE */

/* The density estimator behind the KDE stage.  pisa/utils/kde_hist.py:110-120 calls
 *     k = kde.gaussian_kde(x[D,N], weights=, bw_method=, adaptive=, alpha=);  k(points[D,M])
 * from the external, un-vendored `kde` package (parity of this core is UNPINNED); the
 * estimator object below is what that binding would be replaced by.
 *
 * All-pairs Gaussian kernel sums, no cut-off (the plain O(N*M) double loop):
 *   out[j] = sum_i coef[i] * exp(-0.5 * s2[i] * (q_j - x_i)^T inv_cov (q_j - x_i))
 * d_src[dim][n_src], d_qry[dim][n_qry] (dimension-major), h_inv_cov[dim*dim]
 * row-major symmetric, dim <= 3. */
int pisa_hip_kde_eval(int32_t dim, const double *d_src, const double *d_coef, const double *d_s2,
                      int64_t n_src, const double *d_qry, int64_t n_qry, const double *h_inv_cov,
                      double *d_out, void *stream);

#define PISA_HIP_KDE_SILVERMAN 0   /* factor = (n (d+2) / 4)^(-1/(d+4)) */
#define PISA_HIP_KDE_SCOTT 1       /* factor = n^(-1/(d+4))             */

typedef struct pisa_hip_kde pisa_hip_kde;   /* opaque (host object; device data live in the caller's workspace) */

typedef struct pisa_hip_kde_info_t {
    int32_t dim, cells[3];
    int64_t n_src, n_cells;
    double factor;          /* Silverman / Scott factor                         */
    double norm;            /* sqrt(det(2 pi covariance))                       */
    double sum_w;           /* sum of the weights as given                      */
    double mean[3];         /* weighted mean                                    */
    double covariance[9];   /* weighted data covariance * factor^2 (3x3 row-major, zero padded) */
    double inv_cov[9];
    double r_cut;           /* cut-off radius in kernel sigmas (inf: none)      */
    double cell;            /* cell side in kernel sigmas                       */
    int64_t pairs_pilot;    /* kernel evaluations of the pilot estimate (cells summed through their
                             * Hermite series count P^2/23 + 1 per target: same instruction count) */
    int64_t pairs_eval;     /* kernel evaluations of the last pisa_hip_kde_evaluate */
    int32_t n_dense;        /* cells summed through a Hermite series in the pilot estimate */
} pisa_hip_kde_info_t;

/* `gaussian_kde(x, weights, bw_method, adaptive, alpha)`: weighted mean / covariance, bandwidth
 * matrix, and -- if adaptive -- the pilot densities at the sources and the local bandwidths
 * lambda_i = (pilot_i / geometric mean)^-alpha.  d_x[dim][n] dimension-major; d_w[n] may be NULL
 * (equal weights).  `tol` > 0: kernel values below tol are dropped (cell list, cost O(N k));
 * tol = 0: all pairs.  The caller owns `d_work` (>= pisa_hip_kde_workspace_bytes(dim, n) bytes)
 * and must keep its first pisa_hip_kde_resident_bytes(k) bytes untouched while the estimator
 * is in use; the rest may be reused after the call returns.  Synchronises the stream. */
int64_t pisa_hip_kde_workspace_bytes(int32_t dim, int64_t n_src);
int pisa_hip_kde_create(int32_t dim, const double *d_x, const double *d_w, int64_t n,
                        int32_t bw_method, int32_t adaptive, double alpha, double tol,
                        void *d_work, int64_t work_bytes, pisa_hip_kde **out, void *stream);
int64_t pisa_hip_kde_resident_bytes(const pisa_hip_kde *k);
/* `k(points)`: densities (normalised to integral 1) at d_qry[dim][m] -> d_out[m].  d_work: scratch of
 * >= pisa_hip_kde_eval_workspace_bytes(k, m) bytes, free again on return. */
int64_t pisa_hip_kde_eval_workspace_bytes(const pisa_hip_kde *k, int64_t n_qry);
int pisa_hip_kde_evaluate(pisa_hip_kde *k, const double *d_qry, int64_t m, void *d_work,
                          int64_t work_bytes, double *d_out, void *stream);
/* `k(points)` for the points of a lattice  x[d] = h_origin[d] + i_d h_step[d], 0 <= i_d < h_count[d]
 * (host arrays of length dim), d_out[(i_0 n_1 + i_1) n_2 + i_2] -- numpy.meshgrid(indexing="ij")
 * order, the shape in which get_hist evaluates a map (kde_hist.py:122-190: oversampled bin centres
 * of a regular binning, coszen reflection included).  Same values as pisa_hip_kde_evaluate on the
 * written-out points to rounding (<= 1e-12 relative); in 2-D with a cut-off the kernel values along
 * a lattice line come from a two-multiplication recurrence instead of one exponential each.
 * d_work >= pisa_hip_kde_lattice_workspace_bytes(k, h_step, h_count) bytes. */
int64_t pisa_hip_kde_lattice_workspace_bytes(const pisa_hip_kde *k, const double *h_step,
                                             const int64_t *h_count);
int pisa_hip_kde_evaluate_lattice(pisa_hip_kde *k, const double *h_origin, const double *h_step,
                                  const int64_t *h_count, void *d_work, int64_t work_bytes,
                                  double *d_out, void *stream);
int pisa_hip_kde_info(const pisa_hip_kde *k, pisa_hip_kde_info_t *info);
/* device pointers into the resident workspace, in the estimator's (cell-sorted) source order:
 * whitened coordinates ys[dim][n], kernel coefficients coef[n], squared inverse local bandwidths s2[n] */
int pisa_hip_kde_arrays(const pisa_hip_kde *k, const double **d_ys, const double **d_coef,
                        const double **d_s2);
int pisa_hip_kde_destroy(pisa_hip_kde *k);
/* The Hermite / local-expansion coefficients and split partial sums live in a grow-only scratch buffer of
 * the library, one per HOST THREAD (an evaluation with several worker threads holds one per worker, up to a
 * few GB each at 1e7 events).  A thread that changes streams waits for the previous stream before the
 * buffer is reused.  This call frees the calling thread's buffer. */
int pisa_hip_kde_release_scratch(void);

/* The estimators of one KDE-stage evaluation in one call (pisa/stages/utils/kde.py:154-293 loops over the
 * containers, kde_hist.py:303-372 over the pid channels: 24 independent estimators at the C3 size, all
 * evaluated on the same lattice of oversampled bin centres).  Job by job the result is that of
 * pisa_hip_kde_create(d_x, w, ...) + pisa_hip_kde_evaluate_lattice(...) with
 * w[k] = nan_to_num(d_weights[d_index ? d_index[k] : k]) (kde_hist.py:104-108); the jobs run side by side on
 * `n_threads` host threads of the library (each with its own stream and grow-only workspace; <= 0: 8), longest
 * first, after everything queued on `stream`; on return all d_out are complete.  Returns the first job error. */
typedef struct pisa_hip_kde_job {
    const double *d_x;        /* [dim][n] sample, dimension-major */
    const double *d_weights;  /* weights of the parent sample, or NULL (unit weights) */
    const int64_t *d_index;   /* n indices into d_weights, or NULL (d_weights has n entries) */
    int64_t n;
    double *d_out;            /* densities at the lattice points, numpy.meshgrid(indexing="ij") order */
    double sum_w;             /* out: sum of the weights used (the map's normalisation, kde_hist.py:107) */
    int64_t pairs_pilot;      /* out: as pisa_hip_kde_info_t */
    int64_t pairs_eval;
    int32_t status;           /* out: PISA_HIP_OK or the job's error */
    int32_t reserved;
} pisa_hip_kde_job;
int pisa_hip_kde_lattice_batch(pisa_hip_kde_job *jobs, int32_t n_jobs, int32_t dim, int32_t bw_method,
                               int32_t adaptive, double alpha, double tol, const double *h_origin,
                               const double *h_step, const int64_t *h_count, int32_t n_threads, void *stream);
/* The same in two steps, for a caller that produces the inputs sample by sample (the stage materialises the
 * event weights of one container while the estimators of the previous ones run): _submit queues the jobs and
 * returns (the job array must stay alive and untouched), _wait returns when every job submitted so far is done;
 * then each job's `status` says how it went. */
int pisa_hip_kde_lattice_submit(pisa_hip_kde_job *jobs, int32_t n_jobs, int32_t dim, int32_t bw_method,
                                int32_t adaptive, double alpha, double tol, const double *h_origin,
                                const double *h_step, const int64_t *h_count, int32_t n_threads, void *stream);
int pisa_hip_kde_lattice_wait(void);
/* returns when THESE jobs (a range of an array handed to _submit) are done -- their `status` and outputs may be read --,
 * whatever else is still queued: the stage copies and folds the densities of one container's estimators while the later
 * containers' are still being built (a job that was never submitted counts as done). */
int pisa_hip_kde_lattice_wait_jobs(const pisa_hip_kde_job *jobs, int32_t n_jobs);
/* The pool threads keep their stream, workspaces and estimator scratch between calls (grow-only, a few hundred MB per
 * thread at C3 sizes).  This call waits for the queued jobs, has every pool thread free what it holds and returns when
 * all have; the next submission allocates again. */
int pisa_hip_kde_pool_release(void);

/* How the 2-D fixed-bandwidth pilot estimate sums its cells (fast Gauss transform; truncation error below
 * the cut-off tolerance): 2 (default) = Hermite series of ALL non-empty source cells translated into one
 * local expansion per target cell, 1 = Hermite series of the cells of >= 24 sources evaluated target by target,
 * 0 = every pair directly; < 0 = query.  Returns the previous setting. */
int pisa_hip_kde_configure(int32_t use_expansion);

/* ------------------------------------------------------------------ metric */

#define PISA_HIP_METRIC_LLH 0          /* stats.py:169-253 */
#define PISA_HIP_METRIC_POISSON_LLH 1  /* stats.py:255-326 */
#define PISA_HIP_METRIC_CHI2 2         /* stats.py:98-167  */
#define PISA_HIP_METRIC_MOD_CHI2 3     /* stats.py:651-695 */
/* pisa_hip_metric only (maps in HBM; the fused tails of the evaluation take the four above) */
#define PISA_HIP_METRIC_CORRECT_CHI2 4          /* stats.py:697-730 */
#define PISA_HIP_METRIC_SIGNED_SQRT_MOD_CHI2 5  /* stats.py:762-786 */
#define PISA_HIP_METRIC_MCLLH_MEAN 6            /* stats.py:328-382, likelihood_functions.py:22-63 (a = 0) */
#define PISA_HIP_METRIC_MCLLH_EFF 7             /* stats.py:384-438 (a = 1) */
#define PISA_HIP_METRIC_CONV_LLH 8              /* stats.py:440-596 */

/* The generalized Poisson-gamma likelihood (stats.py:792-879, arXiv:1902.08831 eq. 91): the identifier of the kind
 * in the bindings.  pisa_hip_metric / pisa_hip_finalize_metric* do NOT accept it (it needs per-container alpha, beta
 * and MC counts, and a workgroup per bin): its entry points are pisa_hip_generalized_poisson_llh and
 * pisa_hip_finalize_gpllh below. */
#define PISA_HIP_METRIC_GENERALIZED_POISSON_LLH 9
/* mixture bins keep their recursion (2 (k + 1) doubles) in LDS up to this data count, beyond it in d_scratch */
#define PISA_HIP_GPLLH_LDS_K 1536
#define PISA_HIP_GPLLH_MAX_CONTAINERS 1024

/* generalized_llh_params (stages/likelihood): Sigma w and Sigma w^2 of the events of every bin, the events of
 * bin b being d_weights[d_index[d_offsets[b] .. d_offsets[b + 1])] (a bin's list may share events with another's).
 * d_status = PISA_HIP_ERR_NEGATIVE if a listed weight is negative. */
int pisa_hip_gpllh_bin_sums(const double *d_weights, const int64_t *d_index, const int64_t *d_offsets,
                            int64_t n_bins, double *d_sumw, double *d_sumw2, int32_t *d_status, void *stream);

/* generalized_llh_params.apply_function per (container, bin), all arrays [n_containers][n_bins] but
 * d_adjust[n_containers] (the containers' mean adjustments): an empty bin (n_mc = 0) gets one pseudo-weight
 * 0.001; mean = Sigma w / n, var_z = Sigma w^2 / n; beta = mean / var_z, alpha = (n + adj) mean^2 / var_z
 * (var_z = 0: beta = 1, alpha = (n + adj) 0.001).  d_weights: the weight sums with the pseudo-weight.
 * d_status = PISA_HIP_ERR_NEGATIVE for a negative input. */
int pisa_hip_gpllh_params(const double *d_sumw, const double *d_sumw2, const double *d_n_mc, const double *d_adjust,
                          int32_t n_containers, int64_t n_bins, double *d_alpha, double *d_beta, double *d_weights,
                          int32_t *d_status, void *stream);

/* generalized_poisson_llh per bin (d_per_bin[n_bins], required) and its plain sum (d_total[1]), from
 * d_weights / d_alpha / d_beta / d_n_mc [n_containers][n_bins] and the data d_actual[n_bins] (k = (int64) data).
 * d_empty[n_bins] (uint8, may be NULL): the bins of the reference's `empty_bins`.  A mixture bin with data count
 * k needs k <= scratch_k; for scratch_k > PISA_HIP_GPLLH_LDS_K, d_scratch holds n_bins * 2 (scratch_k + 1)
 * doubles.  d_status: PISA_HIP_ERR_NEGATIVE (negative data or weights), PISA_HIP_ERR_INVALID (alpha or beta
 * <= 0, k > scratch_k).  d_done[1] (uint32, zero before the first call): the arrival counter of the fixed-order
 * reduction of the total, left at zero again; calls that may run concurrently need counters of their own. */
int pisa_hip_generalized_poisson_llh(const double *d_actual, const double *d_weights, const double *d_alpha,
                                     const double *d_beta, const double *d_n_mc, int32_t n_containers, int64_t n_bins,
                                     const uint8_t *d_empty, double *d_scratch, int64_t scratch_k, double *d_per_bin,
                                     uint32_t *d_done, double *d_total, int32_t *d_status, void *stream);

/* The fused tail of an evaluation with the generalized likelihood, n_points sets of limbs (as
 * pisa_hip_finalize_metric_multi): pisa_hip_hist_finalize + pisa_hip_gpllh_params (d_n_mc [n_containers][n_bins],
 * d_adjust [n_containers], fixed at set-up) + pisa_hip_generalized_poisson_llh in ONE launch, bit for bit the
 * same values.  d_per_bin [n_points][n_bins]; d_scratch: n_points * n_bins * 2 (scratch_k + 1) doubles when
 * scratch_k > PISA_HIP_GPLLH_LDS_K; d_done[n_points] as in pisa_hip_generalized_poisson_llh; total[n_points]. */
int pisa_hip_finalize_gpllh(int64_t *d_limbs, int32_t n_points, int32_t n_containers, int64_t n_bins,
                            double *d_hist, double *d_sumw2, const double *d_actual, const double *d_n_mc,
                            const double *d_adjust, const uint8_t *d_empty, double *d_per_bin, double *d_scratch,
                            int64_t scratch_k, uint32_t *d_done, double *total, int32_t *d_status,
                            int32_t *d_metric_status,
                            int32_t clear_limbs, void *stream);

/* Map.metric / metric_total (pisa/core/map.py:1572-1604): per-bin metric of
 * (actual, expected[, sigma2]) and its nansum.  If n_maps > 1 the expectation
 * and variance are first summed over maps in index order
 * (distribution_maker.py:274-281; map.py:1811-1838 adds variances):
 *     d_expected[n_maps][n_bins], d_sigma2[n_maps][n_bins] (may be NULL).
 * d_per_bin[n_bins] may be NULL.  d_total[1] receives the sum; d_status[1]
 * (int32) is set to PISA_HIP_ERR_NEGATIVE for negative inputs. */
int pisa_hip_metric(int32_t kind, const double *d_actual, const double *d_expected,
                    const double *d_sigma2, int32_t n_maps, int64_t n_bins, double *d_per_bin,
                    double *d_total, int32_t *d_status, void *stream);

/* Trial ensembles: Map.metric_total (pisa/core/map.py:1572-1604: Map.metric + np.nansum) of EVERY data map t
 * against EVERY template k in one call, where the reference loops over both:
 *     d_out[t][k] = nansum_b metric(kind; d_data[t][b], d_expected[k][b], d_sigma2[k][b])
 * for kind = PISA_HIP_METRIC_LLH (stats.py:169-253), _POISSON_LLH (:255-326), _CHI2 (:98-167) and _MOD_CHI2
 * (:651-695), with every rule of pisa_hip_metric: the expectation clipped to SMALL_POS, an llh bin without data
 * dropped with its -mu (the NaN of 0 ln 0 under nansum), chi2's whole-map rule (stats.py:160-163: all
 * |d - mu| < 5 eps -> 0) per (t, k) pair.  d_data [n_trials][n_bins], d_expected and d_sigma2 (may be NULL = zeros;
 * read by mod_chi2 only) [n_templates][n_bins], all finite.
 * form: _DIRECT  one lane per (t, k) pair, the bins in ascending order through the per-bin formula (every kind);
 *       _PRODUCT llh and poisson_llh as a dense contraction on the fp64 matrix cores,
 *                    poisson_llh  (sum_b d ln mu - sum_b mu) - sum_b lgamma(d + 1)
 *                    llh          sum_b (d ln mu - [d > 0] mu) - sum_{b: d > 0} (d ln d - d)
 *                (PISA_HIP_ERR_INVALID with a chi2 kind); its preparation buffers belong to the library, one
 *                set per process as the scratch of pisa_hip_metric: product-form calls on different streams
 *                must not overlap;
 *       _AUTO    the product form where it exists.
 * The bits of entry (t, k) depend on row t of d_data and row k of d_expected / d_sigma2 only: not on the number of
 * rows, their position or how the caller splits trials or templates over calls.
 * d_status[1] (int32, zeroed by the caller) is set to PISA_HIP_ERR_NEGATIVE for a negative datum or expectation.
 * PISA_HIP_ERR_INVALID before any device access: an unknown kind or form, a size outside [1, 2^31 - 1], more than
 * 65535 * 16 templates for the full matrix, a NULL pointer, k0 outside [0, n_templates). */
#define PISA_HIP_ENSEMBLE_AUTO 0
#define PISA_HIP_ENSEMBLE_DIRECT 1
#define PISA_HIP_ENSEMBLE_PRODUCT 2
int pisa_hip_metric_matrix(int32_t kind, int32_t form, const double *d_data, const double *d_expected,
                           const double *d_sigma2, int64_t n_trials, int64_t n_templates, int64_t n_bins,
                           double *d_out, int32_t *d_status, void *stream);

/* The same matrix reduced per trial without being written (the loop over hypotheses of a Feldman-Cousins or
 * goodness-of-fit ensemble, where the reference calls Map.metric_total per pair and keeps the best):
 *     v[t][k]   = d_out[t][k] + d_offset[k]        (d_offset may be NULL: v = d_out)
 *     d_best[t] = max_k v[t][k] for the llh kinds, min_k for the chi2 kinds
 *     d_arg[t]  = the smallest k that attains it
 *     d_at[t]   = v[t][k0]
 * bit for bit what the same reduction over pisa_hip_metric_matrix of the same form gives. */
int pisa_hip_metric_matrix_best(int32_t kind, int32_t form, const double *d_data, const double *d_expected,
                                const double *d_sigma2, const double *d_offset, int32_t k0, int64_t n_trials,
                                int64_t n_templates, int64_t n_bins, double *d_best, int32_t *d_arg, double *d_at,
                                int32_t *d_status, void *stream);

/* The same matrix for the metrics that account for finite MC statistics (csrc/ensemble_mc.hip):
 *     d_out[t][k] = nansum_b w(kind; d_data[t][b], d_expected[k][b], d_sigma2[k][b])
 * for kind = PISA_HIP_METRIC_CORRECT_CHI2, _MCLLH_MEAN, _MCLLH_EFF and _CONV_LLH, w the per-bin value of
 * pisa_hip_metric for that kind with every rule kept (the expectation clipped to SMALL_POS, the mixture's Poisson
 * branch at sigma2 == 0, conv_llh's clips, its 101 shifted nodes, the sum opened at the first positive f_x and
 * max(SMALL_POS, .) under both logarithms).  Whatever depends on a template row or a data row alone is computed once
 * per row by a preparation launch, not once per pair; conv_llh's second term norm_conv_poisson(d, d, s) is taken as
 * what it is on the real numbers, exp(log_poisson(d, d)).  Every sum over bins is one compensated chain in ascending
 * order.  d_data [n_trials][n_bins], d_expected and d_sigma2 (required) [n_templates][n_bins], all finite.
 * The bits of entry (t, k) depend on row t of d_data and row k of d_expected / d_sigma2 only: not on the number of
 * rows, their position or how the caller splits trials or templates over calls.
 * d_status[1] (int32, zeroed by the caller) is set to PISA_HIP_ERR_NEGATIVE for a negative d_sigma2 (every kind) and
 * for a negative datum or expectation (the two mcllh kinds; correct_chi2 and conv_llh only clip).
 * PISA_HIP_ERR_INVALID before any device access: any other kind, a size outside [1, 2^31 - 1], more than 65535 * 16
 * templates for the full matrix, (n_trials + n_templates) * n_bins > 256 * (2^31 - 1), a NULL pointer (d_sigma2
 * included; d_offset may be NULL), k0 outside [0, n_templates).
 * The preparation buffers belong to the library, one set per process: calls on different streams must not overlap. */
int pisa_hip_metric_matrix_mc(int32_t kind, const double *d_data, const double *d_expected, const double *d_sigma2,
                              int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_out,
                              int32_t *d_status, void *stream);

/* Reduced per trial as pisa_hip_metric_matrix_best reduces: best = max over k of d_out[t][k] + d_offset[k] for the
 * three llh kinds, min for correct_chi2; the smallest k that attains it; the value at column k0.  Bit for bit the
 * reduction of pisa_hip_metric_matrix_mc. */
int pisa_hip_metric_matrix_mc_best(int32_t kind, const double *d_data, const double *d_expected,
                                   const double *d_sigma2, const double *d_offset, int32_t k0, int64_t n_trials,
                                   int64_t n_templates, int64_t n_bins, double *d_best, int32_t *d_arg, double *d_at,
                                   int32_t *d_status, void *stream);

/* The pseudo-data of such an ensemble drawn on the device: d_out[t][b] ~ Poisson(d_mu[b]) for n_trials trials of
 * one template row, where the reference draws Map.fluctuate("poisson") per trial from a RandomState
 * (pisa/core/map.py:1098-1254).  A counter-based generator cannot reproduce that stream: this one has its own
 * definition (Philox4x32-10, Salmon et al., SC'11) and a statistical validation in the place of a bit comparison.
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (bin b, first_trial + t, stream_id, attempt j)
 * One block of four words gives two doubles in [0, 1): u = ((w_a >> 5) * 2^26 + (w_b >> 6)) * 2^-53 from (w0, w1)
 * and (w2, w3).  0 < mu < 10: inversion by sequential search on the first double of attempt 0 (at most 255 steps);
 * mu >= 10: Hoermann's transformed rejection (PTRS), one block per attempt, j = 0, 1, ... until a draw is accepted;
 * mu = 0 gives 0, a NaN mean gives NaN and draws nothing.
 * The value of entry (t, b) depends on (seed, stream_id, first_trial + t, b, d_mu[b]) only: not on n_trials, on how
 * the caller splits the trials over calls through first_trial, or on the launch geometry.  stream_id separates the
 * ensembles of one seed (analysis/ensemble.py passes the index of the true point).
 * d_status[1] (int32, zeroed by the caller) is set to PISA_HIP_ERR_NEGATIVE for a negative mean, for +inf and for
 * a mean above 2^52; such an entry is NaN.
 * PISA_HIP_ERR_INVALID before any device access: a NULL pointer, a size outside [1, 2^31 - 1],
 * first_trial + n_trials > 2^32. */
int pisa_hip_poisson_fluctuate(const double *d_mu, int64_t n_bins, int64_t n_trials, uint64_t seed,
                               uint32_t stream_id, uint32_t first_trial, double *d_out /* [n_trials][n_bins] */,
                               int32_t *d_status, void *stream);

/* The four methods of Map.fluctuate (pisa/core/map.py:1118-1254, FLUCTUATE_METHODS) on the same generator: n_trials
 * trials of one template row d_mu with the standard deviations d_sigma (NULL is allowed for the poisson method alone).
 * The normal deviate of entry (t, b) comes from the block with the counter (b, first_trial + t, stream_id, 0xFFFFFFFF)
 * under the same key -- an attempt word the Poisson sampler cannot reach, so the deviate is independent of every
 * Poisson block -- as z = PPND16(u) (Wichura, Algorithm AS 241) of the block's first double taken on the open interval,
 * u = ((w0 >> 6) * 2^26 + (w1 >> 6) + 0.5) * 2^-52.
 *     poisson         as pisa_hip_poisson_fluctuate, bit for bit
 *     scaled_poisson  mu == 0 gives 0; s = (sigma sigma) / mu, k ~ Poisson(mu / s), value k s; a negative mean is an
 *                     error here (the reference returns negative multiples); so is sigma == 0 with mu != 0
 *     gauss           mu + sigma z, not clipped; sigma == 0 gives mu
 *     gauss+poisson   g = max(mu + sigma z, 0), then Poisson(g) from the blocks j = 0, 1, ...; sigma == 0 is the
 *                     poisson entry
 * A NaN mean gives NaN and draws nothing.  d_status[1] is set to PISA_HIP_ERR_NEGATIVE, and the entry is NaN, for a
 * NaN, negative or infinite sigma where it is read, and for a Poisson mean without a draw (negative, +inf, > 2^52).
 * The value of entry (t, b) depends on (seed, stream_id, first_trial + t, b, d_mu[b], d_sigma[b], method) only.
 * PISA_HIP_ERR_INVALID before any device access: as pisa_hip_poisson_fluctuate, an unknown method, a NULL d_sigma
 * with a method that reads it. */
#define PISA_HIP_FLUCT_POISSON 0
#define PISA_HIP_FLUCT_SCALED_POISSON 1
#define PISA_HIP_FLUCT_GAUSS 2
#define PISA_HIP_FLUCT_GAUSS_POISSON 3
int pisa_hip_fluctuate(const double *d_mu, const double *d_sigma /* NULL: poisson only */, int32_t method,
                       int64_t n_bins, int64_t n_trials, uint64_t seed, uint32_t stream_id, uint32_t first_trial,
                       double *d_out /* [n_trials][n_bins] */, int32_t *d_status, void *stream);

/* Pseudo-data of a LINEARISED template whose nuisance parameters fluctuate (csrc/fluctuate_linear.hip; DESIGN.md
 * section 4, "pseudo-data with drawn nuisance truths"): every trial draws the truths of J = n_params parameters from
 * their priors and its data from the template at those truths, on the generator above.
 *   truth  d_eta_true[t][j]: h_scale[j] == 0 gives h_shift[j] (nothing is drawn, the box is not read); otherwise the
 *          first of the candidates h_shift[j] + h_scale[j] z_r, r = 0, 1, ..., that lies inside [h_lower[j],
 *          h_upper[j]], z_r = PPND16(u) of the first double (open interval) of the block with the counter
 *          (0x80000000 + j, first_trial + t, stream_id, r) -- a bin word is at most 2^31 - 2, so no block of an entry
 *          has such a counter.  A truncated normal by rejection.  After 256 refused candidates the last one is held
 *          inside the box and d_status[0] becomes PISA_HIP_FLUCT_TRUTH_EXHAUSTED (a caller that refuses a box with
 *          less than a quarter of the prior's mass never sees it: 0.75^256).
 *   mean   mu_t[b] = d_mu[b] + d_response[0][b] eta[t][0] + ... + d_response[J-1][b] eta[t][J-1], ascending j, every
 *          product and sum rounded: the template of pisa_hip_profiled_metric_matrix at eta.  A NaN d_mu[b] stays NaN;
 *          a negative mu_t[b] becomes 0 and is counted in d_status[1] (a count modulo 2^32, no error).
 *   entry  d_out[t][b] is the entry of pisa_hip_fluctuate for the mean mu_t[b]: _POISSON, _GAUSS or _GAUSS_POISSON.
 *          _SCALED_POISSON is refused (its row rules compare a row's variance with its mean, which moves per trial).
 * With every scale and shift 0 and no negative d_mu the output is pisa_hip_fluctuate's, bit for bit.  An entry and a
 * truth depend on (seed, stream_id, first_trial + t, b or j, the inputs) alone.
 * h_scale, h_shift, h_lower, h_upper: HOST arrays [J]; h_lower / h_upper may be NULL (no bound on that side).
 * d_response [J][n_bins], d_eta_true [n_trials][J], d_status[2] (int32, zeroed by the caller): [0] the error word of
 * pisa_hip_fluctuate (_ERR_NEGATIVE takes precedence over _TRUTH_EXHAUSTED), [1] the number of clipped means.
 * PISA_HIP_ERR_INVALID before any launch: as pisa_hip_fluctuate; n_params outside [1, PISA_HIP_PROFILE_MAX_PARAMS];
 * a scale that is NaN, negative or infinite, a shift that is not finite, a NaN bound, lower > upper; a NULL pointer
 * other than h_lower, h_upper and (for _POISSON) d_sigma. */
#define PISA_HIP_FLUCT_TRUTH_EXHAUSTED 1
int pisa_hip_fluctuate_linear(const double *d_mu, const double *d_sigma /* NULL: poisson only */,
                              const double *d_response, int32_t n_params, const double *h_scale,
                              const double *h_shift, const double *h_lower, const double *h_upper, int32_t method,
                              int64_t n_bins, int64_t n_trials, uint64_t seed, uint32_t stream_id,
                              uint32_t first_trial, double *d_out, double *d_eta_true, int32_t *d_status,
                              void *stream);

/* pisa_hip_fluctuate_linear with CORRELATED truths: those of a fit to an observed map (DESIGN.md section 4,
 * "pseudo-data at nuisances fitted to the observed data").  Every trial draws eta ~ N(h_mean, h_cov) inside the box:
 *   factor h_cov [J][J] (row-major, its lower triangle is read) = L L^T, computed once on the host before the launch.
 *          A coordinate with h_cov[j][j] == 0 is dead (what pisa_hip_profiled_hesse writes for a coordinate held on a
 *          bound): its row and column must be zero, it is never drawn and its truth is h_mean[j].  Plain Cholesky row
 *          by row over the live coordinates in ascending order, every operation rounded on its own.
 *   truth  for the attempt r = 0, 1, ...: z_k = PPND16(u) of the block with the counter (0x80000000 + k, first_trial
 *          + t, stream_id, r) for the live k -- the counters of pisa_hip_fluctuate_linear's truths --, and the
 *          candidate x_j = h_mean[j] + L[j][0] z_0 + ... + L[j][j] z_j over the live k in ascending order, every step
 *          rounded.  The first candidate with EVERY coordinate inside [h_lower[j], h_upper[j]] is d_eta_true[t]: the
 *          whole vector is rejected, which samples the normal truncated to the box.  After 256 refused candidates the
 *          last one is held inside the box coordinate by coordinate and d_status[0] becomes
 *          PISA_HIP_FLUCT_TRUTH_EXHAUSTED.
 *   mean, entry, d_status: as pisa_hip_fluctuate_linear.
 * With a diagonal h_cov the truths (and so the data) are those of pisa_hip_fluctuate_linear with h_scale[j] =
 * sqrt(h_cov[j][j]) and h_shift = h_mean, bit for bit, as long as no candidate of that call is refused.
 * PISA_HIP_ERR_INVALID before any launch: as pisa_hip_fluctuate_linear; a NULL h_mean or h_cov; an entry of h_mean or
 * h_cov that is not finite; a mean outside its box; a NaN bound, lower > upper; a dead coordinate with a non-zero
 * entry in its row or column; a pivot that is <= 0 or NaN (h_cov is not positive definite on its live coordinates). */
int pisa_hip_fluctuate_linear_mvn(const double *d_mu, const double *d_sigma /* NULL: poisson only */,
                                  const double *d_response, int32_t n_params, const double *h_mean,
                                  const double *h_cov /* [n_params][n_params] */, const double *h_lower,
                                  const double *h_upper, int32_t method, int64_t n_bins, int64_t n_trials,
                                  uint64_t seed, uint32_t stream_id, uint32_t first_trial, double *d_out,
                                  double *d_eta_true, int32_t *d_status, void *stream);

/* pisa_hip_fluctuate_linear at truths the caller gives: d_eta [n_trials][J] is an INPUT on the device and no truth is
 * drawn; mean, entry and d_status ([0] the error word, [1] the number of clipped means) are those stated there.  With
 * every row of d_eta equal to h_shift the output is that of pisa_hip_fluctuate_linear with every scale 0, bit for bit.
 * A NaN eta entry gives NaN means, which follow the NaN rule (NaN entries, nothing drawn); an infinite one gives means
 * that are infinite or NaN and follow the rules of such a mean.  _SCALED_POISSON is refused.  PISA_HIP_ERR_INVALID before any launch: as there, and a NULL d_eta. */
int pisa_hip_fluctuate_linear_at(const double *d_mu, const double *d_sigma /* NULL: poisson only */,
                                 const double *d_response, int32_t n_params, const double *d_eta, int32_t method,
                                 int64_t n_bins, int64_t n_trials, uint64_t seed, uint32_t stream_id,
                                 uint32_t first_trial, double *d_out, int32_t *d_status, void *stream);

/* ----------------------------------------------- binned post-histogram stages */

/* d_out[i] = d_x[i] * d_scale[i] * scalar  (d_scale may be NULL = 1), then, if
 * has_floor, v < floor ? floor : v  (NaN stays NaN, as np.clip / the reference's
 * apply_floor_gufunc).  d_out may alias d_x.  Used by
 *   discr_sys.hypersurfaces  weights = clip(weights*hs_scales, 0, inf), errors *= hs_scales
 *                            (pisa/stages/discr_sys/hypersurfaces.py:236-257)
 *   utils.set_variance       manual_variance = weights*scale [floored]
 *                            (pisa/stages/utils/set_variance.py:88-104)
 *   data.csv_icc_hist        weights = count*atm_muon_scale (pisa/stages/data/csv_icc_hist.py:79-84) */
int pisa_hip_bin_scale(const double *d_x, const double *d_scale, double scalar, int32_t has_floor,
                       double floor_value, int64_t n, double *d_out, void *stream);
/* d_out[i] = sqrt(d_x[i])  (set_variance.py:84-86: errors = sqrt(manual_variance)) */
int pisa_hip_bin_sqrt(const double *d_x, int64_t n, double *d_out, void *stream);

/* ------------------------------------------------- services around the path */

#define PISA_HIP_MAX_POLY_TERMS 8

/* Replaces `lookup_indices_vectorized_{1,2,3}d` (pisa/core/bin_indexing.py:46-101): flat bin number (C order) of every
 * event among the bin EDGES of 1-3 dimensions, each dimension by the rule of `find_index`
 * (pisa/core/translation.py:504-553: half-open bins, the last edge inside; NaN counts as below); any dimension below
 * -> -1, else any dimension above -> n_bins.  h_d_sample[d]: device column [n]; h_d_edges[d]: device array of
 * h_n_edges[d] ascending edges. */
int pisa_hip_lookup_indices(const double *const *h_d_sample, const double *const *h_d_edges,
                            const int32_t *h_n_edges, int32_t ndim, int64_t n, int64_t *d_index, void *stream);

/* Replaces the gufunc `apply_probs_vectorized` (pisa/stages/osc/two_nu_osc.py:122-127; `calc_probs` :101-110) for one
 * container: d_weights[i] *= flux[i][1]*(1 - P) (flav 1), flux[i][1]*P (flav 2), flux[i][0] (flav 0), with
 * P = theta * sin^2(1.267 deltam31 L(coszen) / E) -- `theta` enters as the reference passes it (the angle itself).
 * d_nu_flux [n][2]. */
int pisa_hip_two_nu_osc(const double *d_nu_flux, double theta, double deltam31, const double *d_energy,
                        const double *d_coszen, int32_t flav, int64_t n, double *d_weights, void *stream);

/* d_out[i] = norm * d_nominal[i] * (d_energy[i] / pivot)^index  (d_nominal may be NULL = 1): the nominal flux and
 * `apply_sys_loop` of pisa/stages/flux/astrophysical.py:69-72, 121-149. */
int pisa_hip_power_law(const double *d_energy, double pivot, double index, double norm, const double *d_nominal,
                       int64_t n, double *d_out, void *stream);

/* d_out[i] = x + (target - x) * fraction, then np.clip(lo, hi) if has_clip; target = d_target[i] or, where d_target
 * is NULL, target_value (pisa/stages/reco/resolutions.py:74-96).  d_out may alias d_x. */
int pisa_hip_shift_toward(const double *d_x, const double *d_target, double target_value, double fraction,
                          int32_t has_clip, double lo, double hi, int64_t n, double *d_out, void *stream);

/* Replaces `apply_genie_sys` (pisa/stages/xsec/genie_sys.py:103-113), `apply_dis_sys` (xsec/dis_sys.py:196-206) and
 * the weight update of background/atm_muons.py:95-101:
 * d_weights[i] *= max(0, scale * prod_k (1 + (lin_k[i] + quad_k[i] p_k) p_k)), k < n_terms <= PISA_HIP_MAX_POLY_TERMS;
 * h_d_quad, or single entries of it, may be NULL (= 0); scale = 1 where the reference has none. */
int pisa_hip_poly_scale(const double *const *h_d_linear, const double *const *h_d_quad, const double *h_params,
                        int32_t n_terms, double scale, int64_t n, double *d_weights, void *stream);

/* numpy.interp(d_x, x_knots, y_knots) -- what scipy's `interp1d(kind='linear')` evaluates for 1-D float data
 * (background/atm_muons.py:82-87 with the spline of :159-164) -- for ascending knots in device memory.  A finite
 * d_x[i] outside [x_knots[0], x_knots[last]] sets *d_status (int32, may be NULL) and gives NaN: interp1d's
 * bounds_error, which the caller raises. */
int pisa_hip_interp_linear(const double *d_x_knots, const double *d_y_knots, int32_t n_knots, const double *d_x,
                           int64_t n, double *d_out, int32_t *d_status, void *stream);

/* d_out[i] = f(sum_g h_coef[g] * h_d_columns[g][i]), the sum from 0.0 in the order of the columns (the loop over
 * `grad_shift_inplace`, pisa/stages/discr_sys/ultrasurfaces.py:339-356, 362-365); mode 0: exp (us_scales), 1: 1 + sum
 * (`approx_exponential`), 2: the sum itself.  n_columns <= PISA_HIP_MAX_COMBINATION. */
#define PISA_HIP_MAX_COMBINATION 64
int pisa_hip_column_combination(const double *const *h_d_columns, const double *h_coef, int32_t n_columns, int32_t mode,
                                int64_t n, double *d_out, void *stream);

/* The element-wise helpers of pisa/utils/vectorizer.py:44-209 (its gufuncs `scale_gufunc` ... `replace_where_counts_gt_gufunc`):
 *   SCALE out = a*scalar;  MUL out = a*b;  IMUL out *= a;  IMUL_AND_SCALE out *= a*scalar;
 *   ITRUEDIV out /= a (0 where a == 0);  ASSIGN out = a;  POW out = a**scalar;  SQRT out = sqrt(a);
 *   REPLACE_WHERE_COUNTS_GT out = a where b > scalar.   d_out may alias d_a. */
#define PISA_HIP_VEC_SCALE 0
#define PISA_HIP_VEC_MUL 1
#define PISA_HIP_VEC_IMUL 2
#define PISA_HIP_VEC_IMUL_AND_SCALE 3
#define PISA_HIP_VEC_ITRUEDIV 4
#define PISA_HIP_VEC_ASSIGN 5
#define PISA_HIP_VEC_POW 6
#define PISA_HIP_VEC_SQRT 7
#define PISA_HIP_VEC_REPLACE_WHERE_COUNTS_GT 8
int pisa_hip_vector_op(int32_t op, const double *d_a, const double *d_b, double scalar, int64_t n, double *d_out,
                       void *stream);

/* Replaces `decoherence.calc_probs` (pisa/stages/osc/decoherence.py:449-466 over `calc_decoherence_probs` :66-106):
 * d_probability[n][3][3], rows (1, 0, 0), (0, 1 - D, D), (0, D, 1 - D) with the numu disappearance D(E, L) of
 * `_calc_numu_disappearance_prob_3flav` (:229-269; h_coef[k] = |U[2][j]|^2 |U[2][k]|^2, h_gamma[k] in GeV, h_delta[k]
 * in eV^2 for the pairs (1,0), (2,0), (2,1)) or, two_flavor != 0, of `_calc_numu_disappearance_prob_2flav`
 * (:112-139; h_coef[0] = 0.5 sin^2(2 theta23), h_gamma[0] = gamma32 in eV, h_delta[0] = dm32).  d_energy in GeV,
 * d_baseline in km. */
int pisa_hip_decoherence_probs(const double *h_coef, const double *h_gamma, const double *h_delta, int32_t two_flavor,
                               const double *d_energy, const double *d_baseline, int64_t n, double *d_probability,
                               void *stream);

/* -------------------------------------------------------------------- flux */

/* 2-D (azimuth-averaged) Honda flux table prepared for `pisa_hip_flux_2d`
 * (host side: scipy splrep exactly as pisa/utils/flux_weights.py:50-131 builds the
 * integral-preserving band splines).  All pointers are device memory. */
typedef struct pisa_hip_flux_table {
    int32_t n_bands;          /* coszen bands of the table (20)                               */
    int32_t n_knots_e;        /* knots of a band spline in log10(E) (106)                     */
    const double *d_knots_e;  /* [n_knots_e]                                                  */
    const double *d_coef_e;   /* [4][n_bands][n_knots_e-4] cubic B-spline coefficients of the
                                 running integrals; primaries (nue, numu, nuebar, numubar),
                                 bands in ascending coszen                                   */
    int32_t n_knots_cz;       /* knots of the coszen spline = n_bands + 1 + 4                 */
    int32_t enpow;            /* flux_weights.py `enpow` (1)                                  */
    const double *d_knots_cz; /* [n_knots_cz]                                                 */
    const double *d_cardinal; /* [n_knots_cz-4][n_bands+1]: coefficients of the interpolating
                                 cubic splines through the unit vectors at the coszen knots   */
    double cz_step;           /* 0.1 (flux_weights.py:343)                                    */
} pisa_hip_flux_table;

/* `calculate_2d_flux_weights` (pisa/utils/flux_weights.py:267-349) for all four
 * primaries at once, as flux.honda_ip uses it (pisa/stages/flux/honda_ip.py:86-104):
 * d_nu_flux[n][2] = (nue, numu), d_nubar_flux[n][2] = (nuebar, numubar).
 * d_status (int32, may be NULL) is set non-zero if a coszen is outside [-1, 1]
 * (the reference raises ValueError, :318-319). */
int pisa_hip_flux_2d(const pisa_hip_flux_table *h_table, const double *d_true_energy,
                     const double *d_true_coszen, int64_t n, double *d_nu_flux,
                     double *d_nubar_flux, int32_t *d_status, void *stream);

/* `hist.apply_function` with a binned calc_mode (pisa/stages/utils/hist.py:132-160):
 *   hist = (unc*w) @ T, sumw2 = (unc*w)^2 @ T, bin_unc2 = (unc^2*w) @ T
 * d_weights[n_calc], d_unc_weights[n_calc] (NULL = 1); T = `hist_transform` (:69-84, event counts
 * per (calc bin, output bin)) given by its non-zeros grouped by output bin: d_ptr[n_out+1],
 * d_col[nnz] (calc bin), d_val[nnz] (count).  Outputs [n_out], any may be NULL. */
int pisa_hip_transform_apply(const double *d_weights, const double *d_unc_weights, const int32_t *d_ptr,
                             const int32_t *d_col, const double *d_val, int64_t n_out, double *d_hist,
                             double *d_sumw2, double *d_bin_unc2, void *stream);

/* Flux on the oscillation grid (flux stages whose calc_mode is osc.prob3's, e.g. the IceCube 3-year
 * cfgs): the reference looks up nu_flux and prob_e / prob_mu at the same node for every event
 * (container.py:981-1012) and multiplies them per event (prob3.py:621-622).  Here the products are
 * formed per node,
 *   d_out[c][node] = (f_e[c][node] * P_e[c][node], f_mu[c][node] * P_mu[c][node]),
 * h_d_flux_nodes[c] = device pointer to container c's [n_nodes][2] flux, d_pepmu = the gather tables
 * of pisa_hip_prob3_grid[_planned]; d_out[c] is then passed as pisa_hip_container.d_pepmu with the
 * static pair (w0*aeff, w0*aeff) in d_weighted_flux[_q]: a flux systematic costs this launch. */
int pisa_hip_flux_prob_tables(const double *const *h_d_flux_nodes, const int32_t *h_nubar,
                              const int32_t *h_flav, int32_t n_containers, const double *d_pepmu,
                              int64_t n_nodes, double *d_out, void *stream);

/* Refresh of the fused kernel's folded flux column after a flux stage rewrote `nu_flux`
 * (flux stages write container['nu_flux'], pisa/stages/flux/barr_simple.py:100; the reference then
 * multiplies it in every evaluation, prob3.py:621-622):
 *   out[e] = d_static_w[e] * d_flux[d_perm ? d_perm[e] : e][0..1]
 * d_flux[.][2] in the container's own event order, d_perm[n] (int64, may be NULL) the resident
 * order of the engine, d_static_w[n] = initial_weights*weighted_aeff in resident order.
 * layout 0: d_out[n][2] (pisa_hip_container.d_weighted_flux); layout 1: the quad-blocked
 * d_weighted_flux_q (padding entries are left untouched). */
int pisa_hip_fold_flux(const double *d_flux, const int64_t *d_perm, const double *d_static_w,
                       int64_t n, int32_t layout, double *d_out, void *stream);

/* pisa_hip_fold_flux for all containers in one launch; set k is folded exactly like
 * pisa_hip_fold_flux(set k). */
typedef struct {
    int64_t n;
    const double *d_flux;       /* [.][2] container order */
    const int64_t *d_perm;      /* [n] or NULL */
    const double *d_static_w;   /* [n] resident order */
    double *d_out;              /* layout 0: [n][2]; layout 1: quad-blocked */
    int32_t layout;
    int32_t reserved;
} pisa_hip_fold_set;
int pisa_hip_fold_flux_multi(const pisa_hip_fold_set *h_sets, int32_t n_sets, void *stream);

/* `apply_sys_vectorized` (pisa/stages/flux/barr_simple.py:147-233). Flux arrays [n][2]. */
int pisa_hip_barr_simple(const double *d_true_energy, const double *d_true_coszen,
                         const double *d_nu_flux_nominal, const double *d_nubar_flux_nominal,
                         int64_t nubar, double nue_numu_ratio, double nu_nubar_ratio,
                         double delta_index, double Barr_uphor_ratio, double Barr_nu_nubar_ratio,
                         int64_t n, double *d_out, void *stream);

/* The same for all containers of a pipeline in one launch (the stage's loop over containers,
 * pisa/stages/flux/barr_simple.py:83-104, with one set of parameter values): set k is evaluated exactly
 * like pisa_hip_barr_simple(set k) -- same bits.  On the oscillation grid (calc_mode = the binning of
 * osc.prob3, as in the IceCube 3-year cfgs) a container is a few 10^4 nodes and the launches, not the
 * arithmetic, are what a flux systematic costs. */
typedef struct {
    int64_t n;                          /* elements of this container */
    const double *d_true_energy;        /* [n] */
    const double *d_true_coszen;        /* [n] */
    const double *d_nu_flux_nominal;    /* [n][2] */
    const double *d_nubar_flux_nominal; /* [n][2] */
    double *d_out;                      /* [n][2] nu_flux */
    int32_t nubar;                      /* +1 / -1 */
    int32_t reserved;
} pisa_hip_barr_set;
int pisa_hip_barr_simple_multi(const pisa_hip_barr_set *h_sets, int32_t n_sets,
                               double nue_numu_ratio, double nu_nubar_ratio, double delta_index,
                               double Barr_uphor_ratio, double Barr_nu_nubar_ratio, void *stream);

/* A flux systematic moved and the flux is held per event (flux.barr_simple in an event representation,
 * pisa/stages/flux/barr_simple.py:83-104, then multiplied in every evaluation, prob3.py:621-622): ONE pass
 * over the events instead of pisa_hip_barr_simple_multi + pisa_hip_fold_flux_multi.
 * pisa_hip_barr_factors (once per event set): the parts of apply_sys_vectorized (:147-233) that depend on
 *   (E, coszen) only -- d_factors[5][n] = ModFlux(nue), ModFlux(numu), the energy and the zenith factor of
 *   the up/horizontal Gaussian, log(E / E_pivot); d_status (int32, may be NULL) is set if an energy is not
 *   positive and finite (such a set must use the two-pass calls, which keep the reference's answers there).
 * pisa_hip_barr_fold_multi (per moved systematic): every array of a set in the SAME order and layout as
 *   d_out -- the engine's resident order, e.g. the quad-blocked d_weighted_flux_q --
 *   d_out[p] = d_static_w[p] * apply_sys(nominal fluxes[p], factors[p]; parameters): the bits of the two
 *   calls it replaces. */
typedef struct {
    int64_t n;                          /* positions (padding included) */
    const double *d_nu_flux_nominal;    /* [n][2] */
    const double *d_nubar_flux_nominal; /* [n][2] */
    const double *d_factors;            /* [5][n] from pisa_hip_barr_factors */
    const double *d_static_w;           /* [n] initial_weights*weighted_aeff (0 at padding) */
    double *d_out;                      /* [n][2] */
    int32_t nubar;                      /* +1 / -1 */
    int32_t reserved;
} pisa_hip_barr_fold_set;
int pisa_hip_barr_factors(const double *d_true_energy, const double *d_true_coszen, int64_t n,
                          double *d_factors, int32_t *d_status, void *stream);
int pisa_hip_barr_fold_multi(const pisa_hip_barr_fold_set *h_sets, int32_t n_sets, double nue_numu_ratio,
                             double nu_nubar_ratio, double delta_index, double Barr_uphor_ratio,
                             double Barr_nu_nubar_ratio, void *stream);

/* ------------------------------------------------------- Fisher matrix and pulls */
/* Replaces the arithmetic of pisa/utils/fisher_matrix.py build_fisher_matrix (:41-75, with get_fisher_matrix
 * :78-116 as its caller) and of pisa/utils/pull_method.py get_derivative_map (:48-86) and calculate_pulls
 * (:131-193, the vector d before the product with the covariance).
 * d_hist / d_sumw2 [n_points][n_rows][n_bins]: n_points templates of n_rows maps each (the rows
 * pisa_hip_hist_finalize writes for n_points * n_containers containers; n_rows = 1: totals already summed).
 * Point 0 is the fiducial.  Per parameter p < n_params <= PISA_HIP_FISHER_MAX_PARAMS (host arrays):
 * the points h_lo[p] < h_hi[p] of its sorted test values and h_dx[p] = hi - lo (finite, non-zero).
 *   T_k[b]    = rows of point k added in ascending index order, starting from row 0 (MapSet.total())
 *   sigma[b]  = sqrt(variances of point 0 added the same way) (Map.std_devs; NOT a variance, as the reference)
 *   g_p[b]    = (T_hi[b] - T_lo[b]) / dx_p                                    -> d_grad [n_params][n_bins]
 *   F_ij      = sum over b with T_0[b] != 0, ascending, from +0.0, of (g_i[b] g_j[b]) / sigma[b]
 *               (one sequential chain per entry: the reference's loop, bit for bit; mirrored, exactly
 *               symmetric)                                                    -> d_matrix [n_params][n_params]
 *   d_p       = the same sum of ((truth[b] - T_0[b]) g_p[b]) / sigma[b]       -> d_pull [n_params]
 *               (d_truth [n_bins] and d_pull both given or both NULL; the reference sums pairwise)
 * d_totals [n_points][n_bins] (may be NULL): the T_k; d_var0 [n_bins] (may be NULL): point 0's variances;
 * d_nonempty[1]: the number of bins with T_0 != 0; d_status[1]: 0, or PISA_HIP_FISHER_ZERO_SIGMA if a nonempty
 * bin has sigma = 0 (maps without errors).  Both are written by the call.  One workgroup: any n_bins.
 * PISA_HIP_ERR_INVALID: an index outside [0, n_points), dx zero or not finite, n_params outside
 * [1, PISA_HIP_FISHER_MAX_PARAMS], n_bins outside [1, 2^31 - 1], sizes that overflow, NULL outputs. */
#define PISA_HIP_FISHER_MAX_PARAMS 32
#define PISA_HIP_FISHER_ZERO_SIGMA 1
int pisa_hip_fisher(const double *d_hist, const double *d_sumw2, int32_t n_points, int32_t n_rows,
                    int64_t n_bins, int32_t n_params, const int32_t *h_lo, const int32_t *h_hi,
                    const double *h_dx, const double *d_truth, double *d_grad, double *d_matrix,
                    double *d_pull, double *d_totals, double *d_var0, int64_t *d_nonempty,
                    int32_t *d_status, void *stream);

/* ------------------------------------------------------- hypersurface fits */
/* Replaces the per-bin loop of pisa/utils/hypersurface/hypersurface.py Hypersurface.fit (:699-959: one Minuit
 * MIGRAD + HESSE per bin on a closure that writes into the object) by ONE launch over n_prob independent
 * problems (bins x maps) that share the design of the systematic sets.
 * Host arrays: h_x [n_par][n_sets] value - nominal per parameter and set (:430; finite); h_form [n_par] one of
 * PISA_HIP_HSFIT_LINEAR ... _LOGARITHMIC (the forms of HYPERSURFACE_PARAM_FUNCTIONS, :81-205; quadratic and
 * exponential_scaled have two coefficients, the others one); h_p0 / h_lo / h_hi / h_inv_prior_sigma [n_coef]
 * start point, bounds (-inf / +inf: none) and prior weights (0: none; :824-839), coefficient 0 the intercept,
 * then every parameter's coefficients in order; n_coef must be 1 + the forms' coefficients.
 * Device arrays: d_y / d_sigma [n_sets][n_prob] the (normalised) maps and their errors, the problem index
 * fastest; d_x [n_par * n_sets] scratch the call fills from h_x on `stream`.
 *   eta_n = c_0 + sum_p f_p(x_pn; c_p);  m_n = exp(eta_n) if log_mode, else eta_n
 *   L(c)  = sum_used ((m_n - y_n) / sigma_n)^2 + sum_i (inv_prior_sigma_i c_i)^2                     (:847-852)
 * A set with sigma_n = 0 is not used, whatever its y and its model value are (:744-749; `include_empty` is the host's: sigma = 1 before upload).  A
 * problem with a non-finite y or sigma among its used sets is not fitted (:781-784); one with fewer used sets
 * than free coefficients is not fitted either (NOT_FITTED | UNDERDETERMINED): coefficients, covariance, chi2 and
 * loss are NaN.  Otherwise Levenberg-Marquardt on the normal equations in fp64 from the start point clamped into
 * the box: damping on the diagonal, a trial point (projected onto the box) is taken only if its loss is finite
 * and not larger, the solve runs over the free components (not the fixed intercept, not a coefficient on a bound
 * whose descent direction leaves the box); stopped when the relative decrease of the loss is <= 1e-10 at a
 * damping lambda <= 1 (a tiny step after a run of refused ones is no stall), else
 * NOT_CONVERGED after max_iter trial points.  Then the EXACT half-Hessian of L (J^T J + sum_n r_n d2r_n + prior)
 * at the point, up to two Newton steps with it, and its inverse by Cholesky:
 *   d_coef [n_prob][n_coef]; d_cov [n_prob][n_coef][n_coef] the covariance HESSE reports with errordef =
 *   LEAST_SQUARES (:917-922), exactly symmetric; NaN with NOT_POSDEF if the half-Hessian is not positive
 *   definite (:921-925); zero rows and columns for a fixed intercept (:956-957) and -- a deviation: Minuit's
 *   error in its transformed space is not meaningful there -- for a coefficient that ends on a bound;
 *   d_chi2 [n_sets][n_prob] ((m - y) / sigma)^2 of EVERY set by plain IEEE division (:982-989);
 *   d_loss, d_n_iter (trial points), d_status [n_prob] (bit flags below).
 * Every matrix entry is one sequential chain over the sets in ascending order: a problem's results do not depend
 * on n_prob, on its place in the batch or on the launch shape.
 * PISA_HIP_ERR_INVALID before any device access: n_par outside [1, MAX_COEFFTS - 1], n_coef not what the forms
 * give or above PISA_HIP_HSFIT_MAX_COEFFTS, n_sets outside [1, PISA_HIP_HSFIT_MAX_SETS], n_prob outside
 * [1, 2^31 - 1] (with the limits no size overflows int64), an unknown form, lo > hi or a NaN bound, x / p0 /
 * prior weight not finite, a negative prior weight or max_iter, a NULL pointer. */
#define PISA_HIP_HSFIT_MAX_COEFFTS 16
#define PISA_HIP_HSFIT_MAX_SETS 128
#define PISA_HIP_HSFIT_LINEAR 0
#define PISA_HIP_HSFIT_QUADRATIC 1
#define PISA_HIP_HSFIT_EXPONENTIAL 2
#define PISA_HIP_HSFIT_EXPONENTIAL_SCALED 3
#define PISA_HIP_HSFIT_LOGARITHMIC 4
#define PISA_HIP_HSFIT_NOT_FITTED 1
#define PISA_HIP_HSFIT_NOT_CONVERGED 2
#define PISA_HIP_HSFIT_NOT_POSDEF 4
#define PISA_HIP_HSFIT_UNDERDETERMINED 8
int pisa_hip_hypersurface_fit(const double *h_x, const int32_t *h_form, int32_t n_par, int32_t n_sets,
                              int64_t n_prob, const double *d_y, const double *d_sigma, const double *h_p0,
                              const double *h_lo, const double *h_hi, const double *h_inv_prior_sigma,
                              int32_t n_coef, int32_t log_mode, int32_t fix_intercept, int32_t max_iter,
                              double *d_x, double *d_coef, double *d_cov, double *d_chi2, double *d_loss,
                              int32_t *d_n_iter, int32_t *d_status, void *stream);

/* ------------------------------------------------------- profiled trial ensembles */
/* pisa_hip_metric_matrix with J = n_params linearised nuisance displacements fitted per (trial, template) pair
 * (csrc/profile.hip; DESIGN.md section 4, "Profiled trial ensembles"):
 *     mu_b(eta) = E[k][b] + R[k][0][b] eta_0 + ... + R[k][J-1][b] eta_(J-1)      (ascending j, every product rounded)
 *     Phi(eta)  = sum_b phi(d_b, mu_b, s2_b) + w sum_j (ips_j (eta_j + c[k][j]))^2
 * phi = mu - d ln mu, w = 1/2 for _LLH and _POISSON_LLH; phi = (d - mu)^2 / mu for _CHI2 and (d - mu)^2 / (s2 + mu)
 * for _MOD_CHI2, w = 1.  eta_hat minimises Phi on the domain mu_b >= 1e-10 for every bin with a non-zero response:
 * a damped Newton iteration from eta = 0 with the exact gradient and Hessian, at most max_iter steps.  The reported
 * entry is the metric of pisa_hip_metric_matrix (_ENSEMBLE_DIRECT) of data row t against the template row
 * mu(eta_hat), then the prior terms w (ips_j (eta_j + c_j))^2 joined in ascending j (subtracted for the llh kinds,
 * added for the chi2 kinds) with the rounding errors kept and added last.
 *   d_response [n_templates][J][n_bins] with response_stride_k >= J n_bins doubles between templates, or ONE
 *       [J][n_bins] block shared by all templates with response_stride_k = 0;
 *   d_inv_prior_sigma [J] (NULL: no priors; an entry 0: no prior on that parameter);
 *   d_center [n_templates][J] the value of parameter j at template k minus its prior mean (NULL: 0);
 *   d_value [T][K]; d_eta [T][K][J] (may be NULL); d_n_iter [T][K] Newton steps taken (may be NULL);
 *   d_pair_status [T][K] bit flags: _NOT_CONVERGED (max_iter steps, or a step that 40 halvings did not make
 *       acceptable), _BOUNDARY (the last step was cut by the domain), _NOT_POSDEF (the Hessian has no Cholesky
 *       factor), _START_OUTSIDE (a responding bin with E < 1e-10: eta stays 0).  A flagged pair still holds the
 *       metric at its last accepted eta.
 * The bits of entry (t, k) depend on row t of d_data and row k of d_expected / d_sigma2 / d_response / d_center
 * alone: not on the number of rows, their order, or how a caller splits them over calls.
 * d_status[1] (int32, zeroed by the caller): PISA_HIP_ERR_NEGATIVE for a negative datum or expectation.
 * PISA_HIP_ERR_INVALID before any device access: an unknown kind, n_params outside [1, _MAX_PARAMS], max_iter
 * outside [0, 4096], a size outside [1, 2^31 - 1], more than 2^26 (strip of 64 trials, template) pairs for the
 * full output or strips for the reduced one (a caller splits the trials or the templates: no entry changes), a response stride that is neither 0 nor >= J n_bins, a NULL pointer where one is required, _MOD_CHI2
 * without d_sigma2, k0 outside [0, n_templates). */
#define PISA_HIP_PROFILE_MAX_PARAMS 8
#define PISA_HIP_PROFILE_NOT_CONVERGED 1
#define PISA_HIP_PROFILE_BOUNDARY 2
#define PISA_HIP_PROFILE_NOT_POSDEF 4
#define PISA_HIP_PROFILE_START_OUTSIDE 8
int pisa_hip_profiled_metric_matrix(int32_t kind, const double *d_data, const double *d_expected,
                                    const double *d_sigma2, const double *d_response, int64_t response_stride_k,
                                    const double *d_inv_prior_sigma, const double *d_center, int32_t n_params,
                                    int32_t max_iter, int64_t n_trials, int64_t n_templates, int64_t n_bins,
                                    double *d_value, double *d_eta, int32_t *d_n_iter, int32_t *d_pair_status,
                                    int32_t *d_status, void *stream);

/* The same entries (+ d_offset[k] per column, may be NULL) reduced per trial as pisa_hip_metric_matrix_best does,
 * the [T][K] matrix never written: d_best / d_arg / d_at, the fitted displacements at both columns d_eta_best and
 * d_eta_at [T][J], and d_trial_status [T] = the pair status at arg OR the pair status at k0.  Bit for bit the
 * reduction of the full output, whatever the sizes.  Where the trials are too few to fill the device the templates
 * are split over workgroups and a second launch joins the ranges through a buffer that belongs to the library (one
 * per process, as the preparation buffers of pisa_hip_metric_matrix): calls on different streams must not overlap. */
int pisa_hip_profiled_metric_matrix_best(int32_t kind, const double *d_data, const double *d_expected,
                                         const double *d_sigma2, const double *d_response, int64_t response_stride_k,
                                         const double *d_inv_prior_sigma, const double *d_center,
                                         const double *d_offset, int32_t k0, int32_t n_params, int32_t max_iter,
                                         int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_best,
                                         int32_t *d_arg, double *d_at, double *d_eta_best, double *d_eta_at,
                                         int32_t *d_trial_status, int32_t *d_status, void *stream);

/* The two entry points above with every displacement fitted inside its range (csrc/profile_bounded.hip; DESIGN.md
 * section 4, "Profiled trial ensembles: bounds"):
 *     eta_hat = argmin Phi(eta)  over  d_lower[k][j] <= eta_j <= d_upper[k][j]  on the same domain.
 * Bounds are displacements in the parameter's units; -inf / +inf: no bound on that side; lower == upper pins the
 * parameter.  The iteration is the same damped Newton iteration with a projected step: it starts at 0 held inside the
 * box (_START_OUTSIDE is judged there), every trial point is held inside the box by comparisons, and after each
 * accepted step the coordinates that sit on a bound with the gradient pointing out of the box leave the Newton system;
 * _NOT_POSDEF and the decrement are those of the remaining block.  A fitted coordinate on a bound holds the bound's
 * own double (eta == bound); no flag marks it, status 0 keeps meaning a clean fit.
 *   d_lower, d_upper [n_templates][J] with bound_stride_k >= J doubles between templates, or ONE [J] block shared by
 *       all templates with bound_stride_k = 0; either may be NULL: no bound on that side.
 *   _BAD_BOUNDS: some j of template k does not satisfy lower <= upper (a NaN bound included).  The pair takes no
 *       step: eta = 0, n_iter = 0, and the entry is the metric at eta = 0.
 * With every bound infinite the outputs are bit for bit those of the entry points above.  Everything said there
 * about placement, d_status, the join buffer (these two entry points have one of their own) and PISA_HIP_ERR_INVALID
 * holds; in addition PISA_HIP_ERR_INVALID for a bound stride that is neither 0 nor >= J. */
#define PISA_HIP_PROFILE_BAD_BOUNDS 16
int pisa_hip_profiled_metric_matrix_bounded(int32_t kind, const double *d_data, const double *d_expected,
                                            const double *d_sigma2, const double *d_response,
                                            int64_t response_stride_k, const double *d_inv_prior_sigma,
                                            const double *d_center, const double *d_lower, const double *d_upper,
                                            int64_t bound_stride_k, int32_t n_params, int32_t max_iter,
                                            int64_t n_trials, int64_t n_templates, int64_t n_bins, double *d_value,
                                            double *d_eta, int32_t *d_n_iter, int32_t *d_pair_status,
                                            int32_t *d_status, void *stream);
int pisa_hip_profiled_metric_matrix_best_bounded(int32_t kind, const double *d_data, const double *d_expected,
                                                 const double *d_sigma2, const double *d_response,
                                                 int64_t response_stride_k, const double *d_inv_prior_sigma,
                                                 const double *d_center, const double *d_lower,
                                                 const double *d_upper, int64_t bound_stride_k,
                                                 const double *d_offset, int32_t k0, int32_t n_params,
                                                 int32_t max_iter, int64_t n_trials, int64_t n_templates,
                                                 int64_t n_bins, double *d_best, int32_t *d_arg, double *d_at,
                                                 double *d_eta_best, double *d_eta_at, int32_t *d_trial_status,
                                                 int32_t *d_status, void *stream);

/* The wide form of the four entry points above: the same fit for up to 32 displacements (csrc/profile_wide.hip;
 * DESIGN.md section 4, "Profiled trial ensembles: more than 8 parameters").  The definition, every argument and every
 * output are those of pisa_hip_profiled_metric_matrix_bounded and pisa_hip_profiled_metric_matrix_best_bounded, with
 * n_params in [1, _WIDE_MAX_PARAMS].  d_lower and d_upper both NULL: the unbounded fit of
 * pisa_hip_profiled_metric_matrix / _best, bit for bit its definition; otherwise the bounded one, _BAD_BOUNDS
 * included.  One wavefront fits one pair, with every sum formed as the same chain in the same order: for
 * n_params <= 8 the outputs are bit for bit those of the entry points they stand in for.
 * PISA_HIP_ERR_INVALID before any device access: as there, with n_params outside [1, 32], and more than 2^26 pairs for
 * the full output or trials for the reduced one.  The join buffer of the reduced form is this pair's own. */
#define PISA_HIP_PROFILE_WIDE_MAX_PARAMS 32
int pisa_hip_profiled_metric_matrix_wide(int32_t kind, const double *d_data, const double *d_expected,
                                         const double *d_sigma2, const double *d_response, int64_t response_stride_k,
                                         const double *d_inv_prior_sigma, const double *d_center,
                                         const double *d_lower, const double *d_upper, int64_t bound_stride_k,
                                         int32_t n_params, int32_t max_iter, int64_t n_trials, int64_t n_templates,
                                         int64_t n_bins, double *d_value, double *d_eta, int32_t *d_n_iter,
                                         int32_t *d_pair_status, int32_t *d_status, void *stream);
int pisa_hip_profiled_metric_matrix_best_wide(int32_t kind, const double *d_data, const double *d_expected,
                                              const double *d_sigma2, const double *d_response,
                                              int64_t response_stride_k, const double *d_inv_prior_sigma,
                                              const double *d_center, const double *d_lower, const double *d_upper,
                                              int64_t bound_stride_k, const double *d_offset, int32_t k0,
                                              int32_t n_params, int32_t max_iter, int64_t n_trials,
                                              int64_t n_templates, int64_t n_bins, double *d_best, int32_t *d_arg,
                                              double *d_at, double *d_eta_best, double *d_eta_at,
                                              int32_t *d_trial_status, int32_t *d_status, void *stream);

/* The wide pair with the form of the nuisance response as an argument (csrc/profile_loglinear.hip; DESIGN.md section
 * 4, "Profiled trial ensembles: the log-linear response").  form = _RESPONSE_LINEAR is the call of the _wide entry
 * point, bit for bit.  form = _RESPONSE_LOGLINEAR reads d_response as rho and fits
 *     mu_b(eta) = E[k][b] exp( rho[k][0][b] eta_0 + ... + rho[k][J-1][b] eta_(J-1) )
 * (the exponent from 0 in ascending j, every product rounded; exp and the product with E rounded once each).  A bin
 * with E == 0 or every rho == 0 does not respond: mu_b = E[k][b] exactly.  A responding bin whose mu is not finite or
 * below 1e-10 puts the trial point outside the domain, and the damping halves the step as for a linear bin below
 * 1e-10: an overflowing exp is a rejected trial point.  Gradient and Hessian are the exact ones of this model,
 *     g_j = sum_b (phi' mu) rho_jb,    H_ij = sum_b (phi'' mu^2 + phi' mu) rho_ib rho_jb,
 * and everything else -- priors, bounds, the Newton state machine, the stop rule, the status flags, the reported
 * metric on mu(eta_hat), the reduced output and its join (through a buffer of this pair's own), placement, d_status
 * -- is what the _wide pair states.  PISA_HIP_ERR_INVALID before any device access: as there, and for a form that is
 * neither of the two. */
#define PISA_HIP_RESPONSE_LINEAR 0
#define PISA_HIP_RESPONSE_LOGLINEAR 1
int pisa_hip_profiled_metric_matrix_wide_form(int32_t kind, int32_t form, const double *d_data,
                                              const double *d_expected, const double *d_sigma2,
                                              const double *d_response, int64_t response_stride_k,
                                              const double *d_inv_prior_sigma, const double *d_center,
                                              const double *d_lower, const double *d_upper, int64_t bound_stride_k,
                                              int32_t n_params, int32_t max_iter, int64_t n_trials,
                                              int64_t n_templates, int64_t n_bins, double *d_value, double *d_eta,
                                              int32_t *d_n_iter, int32_t *d_pair_status, int32_t *d_status,
                                              void *stream);
int pisa_hip_profiled_metric_matrix_best_wide_form(int32_t kind, int32_t form, const double *d_data,
                                                   const double *d_expected, const double *d_sigma2,
                                                   const double *d_response, int64_t response_stride_k,
                                                   const double *d_inv_prior_sigma, const double *d_center,
                                                   const double *d_lower, const double *d_upper,
                                                   int64_t bound_stride_k, const double *d_offset, int32_t k0,
                                                   int32_t n_params, int32_t max_iter, int64_t n_trials,
                                                   int64_t n_templates, int64_t n_bins, double *d_best,
                                                   int32_t *d_arg, double *d_at, double *d_eta_best,
                                                   double *d_eta_at, int32_t *d_trial_status, int32_t *d_status,
                                                   void *stream);

/* The covariance of the fitted displacements (csrc/profile_hesse.hip; DESIGN.md section 4, "Profiled trial ensembles:
 * covariance and pulls"): for trial t, its template k_t = d_k_of_trial[t] (the d_arg of the reduced fit; NULL: k0 for
 * every trial) and the point d_eta[t] ([n_trials][J]; normally d_eta_best or d_eta_at of that fit), one sweep over the
 * bins in ascending order forms gradient and Hessian H of Phi at eta exactly as the solver does, prior terms included.
 *   unbounded (d_lower and d_upper NULL)  d_cov[t] = c H^-1 by the solver's Cholesky factorisation and pivot rule;
 *       c = 1 for _LLH and _POISSON_LLH (Phi is -ln L), c = 2 for _CHI2 and _MOD_CHI2 (Phi is chi2).
 *   bounded   eta is held inside the box of template k_t; the coordinates on a bound with the gradient pointing out of
 *       the box, and the pinned ones, leave the system as in the fit: their rows and columns of d_cov are 0,
 *       d_trial_status[t] has _HELD, and the free block is inverted.  With every bound infinite: the unbounded bits.
 *   d_trial_status [n_trials]: 0, _HELD, or a flag with its meaning above and a NaN covariance: _NOT_POSDEF (the
 *       free block has no Cholesky factor), _START_OUTSIDE (eta is outside the domain: a responding bin with
 *       mu < 1e-10), _BAD_BOUNDS.
 *   d_cov [n_trials][J][J], symmetric bit for bit, written in full.
 * The bits of row t depend on row t of d_data, row k_t of d_expected / d_sigma2 / d_response / d_center / the bounds
 * and d_eta[t] alone.  d_status[1] (int32, zeroed by the caller): PISA_HIP_ERR_NEGATIVE for a negative datum or
 * expectation in a row that is read; PISA_HIP_ERR_INVALID for a k_t outside [0, n_templates) (that row is NaN, its
 * status -1).  PISA_HIP_ERR_INVALID before any device access: as pisa_hip_profiled_metric_matrix_best_bounded where
 * the arguments are the same ones; k0 is checked where d_k_of_trial is NULL; a NULL d_eta, d_cov or d_trial_status;
 * more than 2^32 trials' lanes. */
#define PISA_HIP_PROFILE_HELD 32
int pisa_hip_profiled_hesse(int32_t kind, const double *d_data, const double *d_expected, const double *d_sigma2,
                            const double *d_response, int64_t response_stride_k, const double *d_inv_prior_sigma,
                            const double *d_center, const double *d_lower, const double *d_upper,
                            int64_t bound_stride_k, int32_t n_params, int64_t n_trials, int64_t n_templates,
                            int64_t n_bins, const int32_t *d_k_of_trial /* NULL: k0 */, int32_t k0,
                            const double *d_eta, double *d_cov, int32_t *d_trial_status, int32_t *d_status,
                            void *stream);

/* Samples of the posterior of the displacements, p(eta | data row, template row) (csrc/posterior.hip; the definition:
 * csrc/posterior_device.hpp and DESIGN.md section 4, "Trial ensembles: the nuisance posterior"): a Goodman-Weare
 * stretch-move ensemble sampler (scale a = 2, red-blue split), every problem and every step in one launch.
 * Problem p: data row t_p = d_t_of_problem[p], template row k_p = d_k_of_problem[p] (either NULL: p itself) and
 * W = n_walkers walkers in J = n_params dimensions; H = W / 2.
 *   log-density  lp(eta) = -Phi(eta) for _LLH and _POISSON_LLH, -Phi(eta) / 2 for _CHI2 and _MOD_CHI2, with Phi the
 *       objective stated at pisa_hip_profiled_metric_matrix, formed as the solver forms it at a trial point: bins in
 *       ascending order, a bin with a non-finite datum or expectation skipped, a compensated chain, then the prior
 *       terms in ascending j.  lp = -inf where a responding finite bin has a mean that is not >= 1e-10, where some
 *       eta_j lies outside [lower_j, upper_j] (the arguments of the bounded fit; NULL: no bound), or Phi is NaN.
 *   numbers  Philox4x32-10 under the key of seed, as pisa_hip_fluctuate.  Walker w at step s reads the blocks with the
 *       counters A = (0xC0000000 + w, s, stream_id, chain_id_p) and B = (0xD0000000 + w, s, stream_id, chain_id_p);
 *       chain_id_p = d_chain_id[p] (NULL: p).  u_z and u_p: the first and second double of A on [0, 1) (53 bits of two
 *       words each); u_a: the first double of B on the open interval, as the normal deviates take it.  s = first_step
 *       + i is the GLOBAL step number.  No other block of the library has a first word of this form.
 *   step  the walkers [0, H) move against the current state of [H, W), then [H, W) against the new state of [0, H).
 *       A moving walker at x: z = ((u_z + 1)(u_z + 1)) / 2, the partner q = min((int)(u_p H), H - 1) of the other half
 *       at c, the proposal y_j = c_j + z (x_j - c_j), every operation rounded on its own; accepted iff lp(y) is
 *       neither NaN nor -inf and log(u_a) < (N - 1) log(z) + (lp(y) - lp(x)), N the number of coordinates that are
 *       not pinned (lower_j < upper_j, or an infinite bound).
 *   start  d_x0 [P][W][J].  d_problem_status[p]: _START_OUTSIDE if a walker starts at lp = -inf or NaN, _BAD_BOUNDS for
 *       a bound pair that is not lower <= upper, -1 for a row index outside its array (d_status[0] becomes
 *       PISA_HIP_ERR_INVALID); such a problem does not move, its outputs are NaN and its accept counts 0.
 *   kept  step s iff s >= keep_from and (s - keep_from) % thin == 0; n_keep must be their number among the n_steps.
 *   d_chain [P][n_keep][W][J], d_logp [P][n_keep][W], d_accepted [P][W] (int32: accepted proposals of this call),
 *   d_x_end [P][W][J] (may be NULL): the state after the last step.
 * The bits of problem p depend on its rows, its start, (seed, stream_id, chain_id_p) and the step numbers alone: not
 * on P, the problem's place, the launch, or how the steps are split over calls -- a call of n steps continued from
 * d_x_end with first_step + n equals one call of 2 n steps.
 * d_status[1] (int32, zeroed by the caller): PISA_HIP_ERR_NEGATIVE for a negative datum or expectation in a row that
 * is read.  PISA_HIP_ERR_INVALID before any device access: an unknown kind (the MC-uncertainty kinds have no form
 * here), J outside [1, _MAX_PARAMS], W odd, < 2, < 2 J or > _MAX_WALKERS, thin < 1, a negative first_step or keep_from,
 * first_step + n_steps > 2^32, a size outside [1, 2^31 - 1], a wrong n_keep, a chain of more than 2^40 bytes, a
 * stride as in the bounded fit, a NULL pointer where one is required (d_chain and d_logp unless n_keep is 0),
 * _MOD_CHI2 without d_sigma2, more problems than rows where an index array is NULL. */
#define PISA_HIP_POSTERIOR_MAX_WALKERS 256
int pisa_hip_posterior_sample(int32_t kind, const double *d_data, const double *d_expected, const double *d_sigma2,
                              const double *d_response, int64_t response_stride_k, const double *d_inv_prior_sigma,
                              const double *d_center, const double *d_lower, const double *d_upper,
                              int64_t bound_stride_k, int32_t n_params, int64_t n_data, int64_t n_templates,
                              int64_t n_bins, int64_t n_problems, const int32_t *d_t_of_problem,
                              const int32_t *d_k_of_problem, const uint32_t *d_chain_id, int32_t n_walkers,
                              const double *d_x0, uint64_t seed, uint32_t stream_id, int64_t first_step,
                              int64_t n_steps, int64_t keep_from, int64_t thin, int64_t n_keep, double *d_chain,
                              double *d_logp, int32_t *d_accepted, double *d_x_end, int32_t *d_problem_status,
                              int32_t *d_status, void *stream);

/* ------------------------------------------------------- raw device memory */
/* Thin wrappers so hosts without torch (a cgo/ctypes binding of the
 * reference) can own device buffers. */
int pisa_hip_malloc(void **d_ptr, int64_t bytes);
int pisa_hip_free(void *d_ptr);
int pisa_hip_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes, void *stream);
int pisa_hip_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes, void *stream);
int pisa_hip_memset(void *d_dst, int value, int64_t bytes, void *stream);
int pisa_hip_stream_synchronize(void *stream);
int pisa_hip_set_device(int device);

#ifdef __cplusplus
}
#endif
#endif /* PISA_HIP_H */
