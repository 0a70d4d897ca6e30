/*
 * cgic_hip.h -- C ABI of libcgic_hip.so: the MI355X (gfx950) implementation of
 * Control-GIC's granularity-adaptive VQ + router + entropy-coder hot path.
 *
 * The reference (lianqi1008/Control-GIC) is pure Python and has no FFI layer;
 * its boundary for this path is a set of Python classes.  Each entry point
 * below replaces the body of one of those reference methods (cited as
 * file:line relative to the reference root) and is what a binding for that
 * method would call -- see INTEGRATION.md for the ctypes stubs.
 *
 * Conventions
 *  - Plain C: pointers + sizes, no torch / HIP types.  `stream` is a
 *    hipStream_t passed as void* (NULL = the default stream).
 *  - Pointers documented "device" must be device-accessible allocations on
 *    the current HIP device; everything else is host memory.
 *  - All device work is enqueued on `stream`; no entry point synchronises the
 *    host unless its comment says so.  Outputs are written by the kernels on
 *    that stream; inputs are never modified.
 *  - Return value: CGIC_OK (0) or a negative CGIC_ERR_* code; a message for
 *    the calling thread's last error is available from cgic_last_error().
 *  - Tensors are dense row-major ("contiguous") in the layouts the reference
 *    uses (NCHW images/latents, [K,C] codebook).
 */
#ifndef CGIC_HIP_H
#define CGIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGIC_ABI_VERSION 23

#define CGIC_OK 0
#define CGIC_ERR_INVALID (-1)     /* bad argument (shape, ratio, NULL pointer ...) */
#define CGIC_ERR_UNSUPPORTED (-2) /* valid for the reference, not built here (e.g. e_dim != 4) */
#define CGIC_ERR_HIP (-3)         /* a HIP runtime call failed (no device, launch error ...) */
#define CGIC_ERR_NOMEM (-4)
#define CGIC_ERR_CAPACITY (-5)    /* an output / workspace buffer is too small */

typedef void *cgic_stream_t;

/* number of .bin streams compress() can write per image, in this order
 * (CGIC/models/model.py:226-231): indices_coarse, indices_medium,
 * indices_fine, mask_coarse, mask_medium */
#define CGIC_NUM_STREAMS 5

/* Launch resources: kernels whose workgroups hand work to each other (the VQ loss hand-off, the split index streams of
 * grids beyond 64x64 in compress / decompress) use self-resetting ticket slots in library-owned device memory.  Eager
 * launches take them from a ring that belongs to their stream.  Launches being captured into a hipGraph take them from a
 * pool of 262 144 slots per device and keep them while the graph may still be replayed: a VQ launch takes 1 slot, a
 * split-stream compress 6 per image, a split-stream decompress 3 per image (a compress of more than 682 such images falls
 * back to unsplit streams, a decompress of more than 1365 images is cut into several launches).  The caller says when a captured graph is gone:
 *   id = cgic_ticket_scope_begin();  ... capture (on this thread) ...;  cgic_ticket_scope_end();
 *   ... replay for as long as needed ...;  destroy the graph;  cgic_ticket_scope_release(id);     -> slots returned
 * Captures made outside a scope keep their slots for the life of the process (CGIC_ERR_INVALID once the pool is used up).
 * Call each entry point once eagerly on a device before capturing it (allocations and function attributes are set up on
 * first use).  cgic_ticket_scope_begin / _end return the scope id, _release the number of slots returned, _slots_in_use the
 * captured slots currently held on the current device; all return CGIC_ERR_* (< 0) on misuse. */
int cgic_ticket_scope_begin(void);
int cgic_ticket_scope_end(void);
int cgic_ticket_scope_release(int scope);
int cgic_ticket_slots_in_use(void);
/* test tool: synchronises the device and counts the 32-bit words of the current device's ticket memory (every stream's ring + the used
 * part of the pool for captured launches) that are not zero -- 0 whenever nothing is in flight (every user hands its slots back zeroed);
 * < 0: CGIC_ERR_* */
long long cgic_ticket_pool_dirty_words(void);
int cgic_ticket_pool_dirty_dump(unsigned int *out4, int cap);      /* (dev) the first `cap` of them as (where, slot, word, value) */
/* Launch n captured hipGraphs in one call: graph_execs[i] (hipGraphExec_t) on streams[i] (hipStream_t), in order, back to back on the
 * calling thread.  For runtimes of several independent streams of batches (pipeline.LaneStream): from Python every launch is an
 * interpreter round trip and the last lane starts ~100 us after the first. */
int cgic_launch_graphs(void *const *graph_execs, void *const *streams, int n);
/* Launch groups (ABI 6): independent sub-batches of DIFFERENT shapes through ONE launch per kernel.  The reference cuts a high-
 * resolution image into a 768-px grid with a ragged last row / column (inference_high_resolution.py:112-125) and runs
 * model.compress on the tiles one after the other (:236-257); tiles of equal shape are one batch here, but a 2040x1356
 * image is still four shapes = four launch chains.  Between cgic_group_begin(n, shares) and cgic_group_launch(stream) the calls
 * of THIS thread to cgic_entropy_maps_f32 / _u8, cgic_vq_forward_route_f32, cgic_index_histogram, cgic_compress_streams and
 * cgic_decompress_streams check
 * their arguments and record their launches instead of making them (cgic_group_select(g) says which group the following calls belong
 * to; within a group the calls are dependent in call order, across groups nothing is); cgic_group_launch then issues the j-th
 * launches of all groups as ONE launch whose grid is the concatenation of theirs (each workgroup finds its group's argument block
 * from its block index), j = 0, 1, ...  Other entry points, and positions where the groups recorded different kernels, are
 * launched one by one: results never depend on the grouping.  Outputs of recorded calls are written when cgic_group_launch's
 * launches run: nothing else may be enqueued on them in between, and every device buffer handed to a recorded call (inputs,
 * outputs, workspaces) must stay allocated until cgic_group_launch has returned.
 *   shares  host [n] or NULL: each group's share of the chip (sums to ~1; e.g. its share of the latent vectors): the
 *           persistent-workgroup VQ launch of a group takes that share of the CUs.  NULL: 1/n each.
 * cgic_group_launch returns the number of launches issued (>= 0) or CGIC_ERR_*; the group is closed either way.  `stream` must be
 * the stream the recorded calls were given (positions without a grouped form are launched on the stream they recorded).
 * cgic_group_abort closes it without launching.  cgic_group_max: the largest n. */
int cgic_group_max(void);
int cgic_group_begin(int ngroups, const double *shares);
int cgic_group_select(int group);
int cgic_group_launch(cgic_stream_t stream);
void cgic_group_abort(void);
const char *cgic_last_error(void);
int cgic_abi_version(void);
/* number of visible HIP devices, or CGIC_ERR_HIP; never throws, never aborts */
int cgic_device_count(void);

/* ---------------------------------------------------------------------------
 * A. VectorQuantize2.forward -- CGIC/modules/vqvae/quantize.py:69-97
 *
 *   z        device [B, 4, hw]  fp32 (NCHW latent, hw = h*w)
 *   codebook device [K, 4]      fp32 (embedding.weight; K % 16 == 0, K <= 8192)
 *   indices  device [B*hw]      int64   argmin_k ||z - e_k||^2 with the CPU
 *            reference's fp32 rounding sequence; lowest index on exact ties
 *   z_q      device [B, 4, hw]  fp32 or NULL   = z + (e[idx] - z)      (:93)
 *   loss     device [1]         fp32 or NULL   = m + beta*m, m = mean((e[idx]-z)^2)
 *            (:85-90; legacy=1 -> m + beta*m, legacy=0 -> beta*m + m)
 *   hist     device [K]         int64 or NULL  += occurrences of each index
 *            (the usage counter of quantize.py:28,79-81, exact integers)
 *   workspace device, cgic_vq_workspace_bytes(B*hw) bytes, or NULL iff loss==NULL
 *   quant_conv NULL, or the 1x1 convolution in front of the quantiser (CGIC.quant_conv, model.py:51,110) to apply to
 *            every latent vector first: then `z` is the encoder output h and everything above refers to W h + b
 *   prepared NULL, or the image cgic_vq_prepare_f32 made of THIS codebook (16-byte aligned, cgic_vq_prepared_bytes(K)
 *            bytes): what every workgroup otherwise derives from `codebook` at the head of every launch (row norms, the
 *            maxima that fix the fp16 scaling, the split operands of the candidate filter: torch.sum(embedding.weight**2)
 *            of quantize.py:73-75 is recomputed by the reference on every call as well).  Inference keeps one codebook for
 *            thousands of launches: prepare once, pass it along.  The caller re-prepares when the weights change
 *            (VectorQuantize2 keys it on the weight's version counter); results are identical with and without it.
 * Two implementations behind the same contract, bit-identical results: for K % 64 == 0, K <= 1024 (the reference's
 * 1024 x 4 codebook) an fp16-MFMA candidate filter with an exact fp32 resolve, otherwise the fp32-MFMA loop over
 * every code (no fused quant_conv there: CGIC_ERR_UNSUPPORTED).
 * Non-finite values: torch.argmin returns the first NaN; here a NaN distance never wins (lowest index among the
 * minimal non-NaN distances, 0 if all are NaN).  The deviation is confined to vectors whose own distance row
 * contains a non-finite value (tests/test_gpu_stress.py).
 * ------------------------------------------------------------------------- */
/* torch.nn.Conv2d(4, 4, 1) as the CPU reference computes it: per output channel an fma chain over the input
 * channels in order.  oneDNN seeds the accumulator with the bias or adds it at the end depending on shape and
 * thread count (measured with torch 2.10: 1 thread, or a 64x64 latent -> bias last; 8 threads and >= 96x96 ->
 * bias first); `bias_first` selects which of the two sequences to reproduce. */
/* The pixels behind a pair of entropy maps, for the router's threshold-band refinement (cgic_router_f32 below). */
typedef struct cgic_pixels {
    const void *x;      /* device: the image batch the maps were computed from -- [B, 3, 16 h16, 16 w16] fp32, or, with
                         * is_u8, the uint8 frames [B, 16 h16, 16 w16, 3] of cgic_entropy_maps_u8 (4-byte aligned) */
    int is_u8;
    const float *bins;  /* host [32] fp32: torch.linspace(-1, 1, 32) (model.py:480) */
    int nbins;          /* 32 */
    float sigma;        /* 0.01 (model.py:481) */
    const float *flat8; /* device [B, 2 h16, 2 w16] fp32 or NULL: the flat8 output of the entropy call that made the maps.
                         * Without it constant patches are re-evaluated one by one like any other (same result, slower on
                         * flat content) */
    void *scratch;      /* device, cgic_router_refine_scratch_bytes(...) bytes, or NULL (ABI 7).  With it a long band -- smooth or
                         * flat 8-bit content puts tens to hundreds of patches within the band of a threshold -- is not evaluated
                         * by every router workgroup of the image on its own: cgic_router_f32 publishes it to every idle wave of
                         * the launch (the other row bands of a tile, finished router workgroups); cgic_vq_forward_route_f32 has
                         * the row bands of a large tile (>= 32x32 patches routed per image: up to 8 workgroups) split it between
                         * them -- a smooth 768x768 tile 251 -> 82 us (the routers run the plain code first and start over in
                         * the split code only when a band is long: nothing measurable on an ordinary tile).  Same masks either way.
                         * REQUIRED (ABI 8) when the routing segment does not fit the workgroup's LDS (cgic_router_refine_in_lds == 0: the
                         * flattened batch of the reference's encode(), RouterTriple.py:21,40,52,63, or an untiled image beyond
                         * 768x768): the refinement then runs as a chain of launches over patched copies of the maps kept here.
                         * Uninitialised memory; one per launch in flight, and at most FOUR launches that carry one in flight on a
                         * device at a time (the row bands of a tile wait for each other: all of them must be resident) */
    size_t scratch_bytes;
} cgic_pixels;
/* scratch for cgic_pixels.scratch of a router / fused call with these arguments (0: the call takes none; required when
 * cgic_router_refine_in_lds(...) == 0) */
size_t cgic_router_refine_scratch_bytes(int64_t B, int64_t h16, int64_t w16, int per_image);

typedef struct cgic_conv1x1 {
    const float *weight;   /* device [4, 4] fp32 = Conv2d.weight[:, :, 0, 0], row = output channel */
    const float *bias;     /* device [4] fp32 or NULL */
    int bias_first;
} cgic_conv1x1;
/* out[n] = conv(rows[n]) for n rows of 4 floats (post_quant_conv applied to the codebook, model.py:52,115) */
int cgic_conv1x1_rows_f32(const float *rows, int64_t n, const cgic_conv1x1 *conv, float *out, cgic_stream_t stream);

/* Telemetry of the candidate-filter path (K % 64 == 0, K <= 1024): launches enqueued (or captured) after this call add to
 * device_counters[0..3] (uint32, device memory, zeroed by the caller): [0] vectors whose runner-up tile was inside the
 * margin, so that the wave scanned all K codes exactly for them; [1] 64-vector groups with more than 12 such vectors, rerun
 * on the exact fp32-MFMA loop; [2] groups that evaluated a second 16-code candidate set exactly.  NULL switches it off (the
 * default).  Process-wide; the counters are only touched inside those rare branches.  Results never depend on it. */
int cgic_vq_stats(unsigned int *device_counters);
/* Margin telemetry of the candidate filter: the SAME kernel body as cgic_vq_forward_f32's filter path (K % 64 == 0, K <= 1024),
 * instantiated so that it also writes out what it decided on:
 *   scores device [B*hw, K] fp32: the approximate score f_k = ee_k - 2 z.e_k of every code as the fp16 matrix cores delivered it
 *          (scaled back to score units) -- the exactness argument bounds |f_k - F_k| <= 1.8e-6 (ee_k + 2 sum|z_j e_kj|) + floor
 *   aux    device [B*hw, 6]  fp32: per vector (f_min, the margin M, the candidate threshold f_min + M + floor, 1 if the vector was
 *          sent to the all-K exact scan, the exponent q of its score scaling 2^q, the bound S on ee_k + 2 sum|z_j e_kj|)
 *   indices device [B*hw] int64: the result (identical to cgic_vq_forward_f32's)
 * tools/stress_vq.py --telemetry and tests/test_gpu_stress.py compare the observed error and the margin actually consumed by
 * the reference's winners with the budget.  Not a product path: B*hw*K*4 bytes of output. */
int cgic_vq_filter_probe_f32(const float *z, int64_t B, int64_t hw, const float *codebook, int K, int64_t *indices,
                             float *scores, float *aux, cgic_stream_t stream);
size_t cgic_vq_workspace_bytes(int64_t n_vectors);
/* bytes of the prepared codebook image (0: this K only has the exact loop, which needs none) / make it (one small launch).
 * Near-duplicate rows -- a trained codebook's clusters and dead codes (quantize.py:22-26,78) -- are packed into one 32-code tile of
 * the image each (keys = original index << 16 | position travel with it; ties still go to the lowest ORIGINAL index), so that they
 * do not send every nearby vector to the all-K exact scan.  For that cgic_vq_prepare_f32 copies the K rows (16 KB) to the host and
 * WAITS for `stream` -- once per codebook; while `stream` is being captured it makes the plain image instead (same results). */
size_t cgic_vq_prepared_bytes(int K);
/* the packing itself, host only (no GPU involved; what cgic_vq_prepare_f32 computes from its host copy of the rows): perm[p] = the
 * ORIGINAL row that sits at position p of the image.  Returns 1 and fills perm[0..K), 0 when there is nothing to pack (no two rows
 * within 3e-4 x the largest |entry| of each other under the max-norm: the image is the plain one), CGIC_ERR_* on bad arguments. */
int cgic_vq_cluster_permutation_host(const float *codebook_host, int K, uint16_t *perm_out);
int cgic_vq_prepare_f32(const float *codebook, int K, int e_dim, void *prepared, cgic_stream_t stream);
int cgic_vq_forward_f32(const float *z, int64_t B, int64_t hw, const float *codebook, int K, int e_dim,
                        float beta, int legacy, int64_t *indices, float *z_q, float *loss,
                        int64_t *hist, void *workspace, const cgic_conv1x1 *quant_conv, const void *prepared,
                        cgic_stream_t stream);
/* cgic_vq_forward_f32 and cgic_router_f32 in ONE launch: the router's per-image workgroups share the grid with
 * the VQ workgroups (neither needs the other's output; both need what precedes them, i.e. the latent and
 * the entropy maps).  Same contracts as the two separate calls (`refine`: see cgic_router_f32). */
int cgic_vq_forward_route_f32(const float *z, int64_t B, int64_t hw, const float *codebook, int K, int e_dim,
                              float beta, int legacy, int64_t *indices, float *z_q, float *loss,
                              void *workspace, const float *e16, const float *e8, int64_t h16, int64_t w16,
                              double coarse_ratio, double medium_ratio, int per_image, int32_t *mask_c,
                              int32_t *mask_m, int32_t *mask_f, float *gate, int *mode_out,
                              const cgic_conv1x1 *quant_conv, const void *prepared, const cgic_pixels *refine,
                              cgic_stream_t stream);
/* same contract, plain-VALU kernel (no MFMA); kept as an independent
 * implementation for cross-checking the MFMA kernel's rounding */
int cgic_vq_forward_valu_f32(const float *z, int64_t B, int64_t hw, const float *codebook, int K,
                             int e_dim, float beta, int legacy, int64_t *indices, float *z_q,
                             float *loss, int64_t *hist, void *workspace, const cgic_conv1x1 *quant_conv,
                             cgic_stream_t stream);

/* Backward of cgic_vq_forward_f32 for training (quantize.py:85-93 under autograd, CGIC.training_step model.py:155-174):
 *   g_zq   device [B, 4, hw] fp32 or NULL   gradient arriving at z_q (straight-through: passes to z)
 *   g_loss device [1] fp32 or NULL          gradient arriving at loss
 *   g_z    device [B, 4, hw] fp32 or NULL   = g_zq + g_loss * (-2/n * w_z) * (e[idx] - z)      (bit-identical to that expression)
 *   g_codebook device [K, 4] fp32 or NULL   = g_loss * (2/n * w_e) * sum_{idx[n] = k} (e[idx] - z_n); n = B*hw*4,
 *          (w_z, w_e) = (1, beta) if legacy else (beta, 1).  Deterministic (fixed-point LDS accumulation per workgroup,
 *          workgroup tables added in a fixed order), unlike torch.index_add_'s fp32 atomics.  Workgroup j of
 *          min(256, ceil(N/2048)) takes the vectors [j*per, (j+1)*per), per = ceil(N/workgroups), N = B*hw, and rounds every
 *          difference to a multiple of 2^(e_Mj - 30), e_Mj the exponent of its range's largest |e - z|: a term is
 *          off by at most 2^(e_Mj - 31), the sums are exact, one fp32 rounding at the end.  (A range whose largest
 *          difference is subnormal, below 2^-126, contributes zero.)
 *   g_z is the expression above in IEEE arithmetic (NaN exactly where it is NaN; g_loss = inf: inf * 0 is NaN).  An Inf or
 *          NaN difference makes the codebook gradient of its whole range of vectors meaningless (no contract yet).
 *   B*hw == 0: g_codebook is zeroed, nothing else is touched (z, indices may be NULL).
 *   workspace device, cgic_vq_backward_workspace_bytes(B*hw, K) bytes, or NULL iff g_codebook == NULL */
size_t cgic_vq_backward_workspace_bytes(int64_t n_vectors, int K);
int cgic_vq_backward_f32(const float *z, int64_t B, int64_t hw, const float *codebook, int K, int e_dim,
                         const int64_t *indices, const float *g_zq, const float *g_loss, float beta, int legacy,
                         float *g_z, float *g_codebook, void *workspace, cgic_stream_t stream);

/* usage histogram of an index tensor (quantize.py:79-81): hist[idx[i]] += 1 */
int cgic_index_histogram(const int64_t *indices, int64_t n, int K, int64_t *hist, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * C'. Entropy.forward -- CGIC/models/model.py:433-483, patch sizes 8 and 16 in
 * one pass over the image (CGIC.encode computes both, model.py:100-101).
 *
 *   x     device [B, 3, H, W] fp32, H % 16 == 0, W % 16 == 0
 *   bins  host   [32] fp32  (torch.linspace(-1, 1, 32), model.py:480)
 *   e8    device [B, H/8,  W/8 ] fp32 or NULL
 *   e16   device [B, H/16, W/16] fp32 or NULL
 *   flat8 device [B, H/8,  W/8 ] fp32 or NULL: per 8x8 patch its gray value (0.2989 R + 0.5870 G + 0.1140 B, model.py:471) if
 *         all 64 pixels carry the same one, else NaN -- by-product of the pass, consumed by the router's refinement
 *         (cgic_pixels.flat8): constant patches are the large tie groups of real content
 * fp32 throughout; exp / log / reciprocal are the GPU's (v_exp_f32, v_log_f32, v_rcp_f32) and only the 2 bins
 * that bracket a pixel are evaluated (the rest is <= 9e-10 per pixel), so results match the CPU reference to
 * ~1e-6 (measured <= 1.1e-6; tests hold it to 2e-6), not bit-for-bit (SURVEY.md section 7 "hard parts"); see
 * cgic_entropy_maps_ref_f32 below for the variant that follows the reference's rounding.
 * ------------------------------------------------------------------------- */
int cgic_entropy_maps_f32(const float *x, int64_t B, int64_t H, int64_t W, const float *bins,
                          int nbins, float sigma, float *e8, float *e16, float *flat8, cgic_stream_t stream);
/* The same maps in the REFERENCE'S OWN ARITHMETIC (opt-in): torch's CPU operation sequence and summation order -- gray as three
 * products and two sums, IEEE divide by sigma, the mean over a patch's pixels as torch's cascade sum (chunks of 16 pixels in
 * row-major order, then the chunk sums), both sums over the 32 bins as torch's eight strided partials -- with exp / log
 * correctly rounded (fp64, rounded once).  The router's thresholds are k-th smallest entropies with a strict '<'
 * (RouterTriple.py:21-34), so on tie-heavy content (8-bit, flat, blocky images) the last bits of the maps decide which
 * patches fall under a threshold: against the real Entropy class this variant is bit-identical in 98.6-100 % of the values
 * (the rest within 5e-7: torch's exp / log are MKL's) and flips no mask element on any measured content family, where the
 * default kernel (accurate to ~1e-6, order-free) flips a few elements in ~1 of 64 such images.  ~8x the instructions of
 * the default kernel.  Same arguments and contract as cgic_entropy_maps_f32. */
int cgic_entropy_maps_ref_f32(const float *x, int64_t B, int64_t H, int64_t W, const float *bins,
                              int nbins, float sigma, float *e8, float *e16, cgic_stream_t stream);
/* ToTensor + Entropy in one pass, for frames that arrive as uint8 (the datasets of both scripts: PIL image -> center crop ->
 * T.ToTensor(), inference.py:50-59, then CGIC.encode's two Entropy calls, model.py:99-101).
 *   x_hwc  device [B, H, W, 3] uint8 (PIL / decoder layout), 4-byte aligned, H % 16 == 0, W % 16 == 0
 *   x_out  device [B, 3, H, W] fp32 or NULL: byte / 255 exactly as torch's `.div(255)` rounds it = what ToTensor hands to the
 *          conv encoder (bit for bit, all 256 byte values)
 *   e8, e16 as cgic_entropy_maps_f32 -- and bit-identical to cgic_entropy_maps_f32 run on x_out.
 * 3 B read + 12 B written per pixel instead of ToTensor's 3 + 12 and Entropy's 12 again. */
int cgic_entropy_maps_u8(const unsigned char *x_hwc, int64_t B, int64_t H, int64_t W, const float *bins,
                         int nbins, float sigma, float *x_out, float *e8, float *e16, float *flat8, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * C. TripleGrainFixedEntropyRouter -- CGIC/modules/vqvae/RouterTriple.py:8-95
 *
 * cgic_router_mode: the 7-way mode from the zero-ness of the ratios, with
 * fine = 1 - coarse - medium evaluated in float64 (:13,19,36,72).
 *
 * cgic_router_f32:
 *   e16 device [B, h16, w16] fp32;  e8 device [B, 2*h16, 2*w16] fp32
 *   per_image = 0: thresholds over the flattened batch (the reference, :21,40,52,63)
 *   per_image = 1: one threshold set per image == B independent B=1 calls
 *   mask_c device [B, h16, w16], mask_m [B, 2h16, 2w16], mask_f [B, 4h16, 4w16] int32
 *   gate   device [B, 4h16, 3*4w16] fp32 or NULL  (cat(up4(gc), up2(gm), gf), :93)
 *   mode_out host int or NULL
 * k = round(n*ratio) uses Python's round-half-even on the float64 product.
 * CGIC_ERR_INVALID if k > n (the reference raises IndexError there).
 *
 *   refine NULL: the masks are exactly the reference router's for the maps AS GIVEN (bit-exact integer / compare work).
 *          Non-NULL (round 4; what the pipeline passes by default): the masks are the reference's from the PIXELS.  The
 *          thresholds are k-th smallest entropies compared with a strict '<' (:21-34) and the maps of cgic_entropy_maps_f32
 *          are within ~1e-6 of the reference's arithmetic, not equal to it, so on tie-heavy content (8-bit, smooth, flat
 *          images) the last bits decide masks and hence .bin bytes.  With the pixels, every patch whose entropy lies within
 *          4e-6 (>= twice the kernel's error) of a threshold is re-evaluated inside the router in the reference's own fp32
 *          operation order (the arithmetic of cgic_entropy_maps_ref_f32), and the k-th smallest is taken again: the result
 *          equals routing on cgic_entropy_maps_ref_f32's maps (tested), at the default kernel's cost whenever the band holds
 *          only the threshold element itself -- the typical image.  A segment whose maps fit the workgroup's LDS
 *          (per-image routing of images / tiles up to 768x768, batch-global routing of a few images:
 *          cgic_router_refine_in_lds) is refined inside the router's workgroup; a larger one (ABI 8: the flattened batch of
 *          the reference's encode(), RouterTriple.py:21,40,52,63; an untiled large image) through patched copies of the
 *          maps in refine->scratch (five launches; not inside a launch group: CGIC_ERR_UNSUPPORTED).  The maps themselves
 *          are not modified.
 * ------------------------------------------------------------------------- */
int cgic_router_mode(double coarse_ratio, double medium_ratio);
/* 1 if cgic_router_f32 / cgic_vq_forward_route_f32 accept `refine` for this shape (ABI 8: every shape whose segment has fewer
 * than 2^31 patches), else 0 */
int cgic_router_refine_supported(int64_t B, int64_t h16, int64_t w16, int per_image);
/* 1 if the segment is refined inside the router's workgroup (its maps fit the LDS); 0: through refine->scratch (see above) */
int cgic_router_refine_in_lds(int64_t B, int64_t h16, int64_t w16, int per_image);
int cgic_router_f32(const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16,
                    double coarse_ratio, double medium_ratio, int per_image, int32_t *mask_c,
                    int32_t *mask_m, int32_t *mask_f, float *gate, int *mode_out,
                    const cgic_pixels *refine, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * D. HuffmanCoding.__init__ / make_heap / merge_nodes / make_codes --
 * CGIC/tools/indices_coding.py:10-17,46-75 (host side; CPython heapq
 * tie-breaking reproduced exactly).
 *
 *   freq  host [n] int64  int(value.item()) per symbol: none negative, their
 *         sum below 2^62
 *   order host [n] int32 or NULL: order[i] = symbol pushed i-th = iteration
 *         order of the `frequency` mapping (NULL = 0,1,2,...).  NB the
 *         reference's mapping is an nn.ParameterDict built from a plain dict
 *         (quantize.py:28) and therefore iterates its keys sorted AS STRINGS.
 * The table owns host copies and (lazily, per device) device copies.
 * cgic_table_binary(): the fixed table {0:'0', 1:'1'} of BinaryCoding
 * (CGIC/tools/mask_coding.py:11-12).
 * ------------------------------------------------------------------------- */
typedef struct cgic_table cgic_table;
int cgic_table_create(const int64_t *freq, const int32_t *order, int n, cgic_table **out);
int cgic_table_binary(cgic_table **out);
void cgic_table_destroy(cgic_table *t);
int cgic_table_num_symbols(const cgic_table *t);
int cgic_table_max_len(const cgic_table *t);
int cgic_table_words(const cgic_table *t); /* 32-bit words per code = ceil(max_len/32) */
/* host copies: len [n] int32 bits; code [n*words] uint32, bit i of a code is
 * bit 31-(i%32) of word i/32 (MSB first) */
int cgic_table_get(const cgic_table *t, int32_t *len, uint32_t *code);

/* ---------------------------------------------------------------------------
 * E/F. single-stream coders: HuffmanCoding.compress / decompress_string
 * (indices_coding.py:113-126,153-168) and BinaryCoding.compress /
 * decompress_string (mask_coding.py:40-55,81-96), minus the file I/O which
 * stays in the Python host.
 *
 * cgic_encode_stream:
 *   syms   device [n] int64 (a table with 2 symbols also accepts int32 via
 *          elem_bytes = 4: BinaryCoding is fed int32 masks, model.py:230)
 *   out    device [cap] uint8; framing: 1 byte pad count (1..8), code bits
 *          MSB-first, pad zero bits; n == 0 -> 0 bytes (empty file)
 *   nbytes device [1] int32: bytes produced, or CGIC_ERR_* (<0) if a symbol
 *          is outside the table (KeyError in the reference) / cap too small;
 *          `out` must be 4-byte aligned
 * cgic_decode_stream:
 *   in     device [nbytes] uint8 (+ >= 8 readable bytes of slack after it)
 *   syms   device [cap] int64; count device [1] int64: symbols decoded, or -1
 *          for an empty input (the reference returns None)
 * Workspace: cgic_stream_workspace_bytes(n) for encode; decode needs none.
 * ------------------------------------------------------------------------- */
size_t cgic_stream_capacity(const cgic_table *t, int64_t n_symbols);
size_t cgic_stream_workspace_bytes(int64_t n_symbols);
int cgic_encode_stream(const cgic_table *t, const void *syms, int elem_bytes, int64_t n, uint8_t *out,
                       int64_t cap, int32_t *nbytes, void *workspace, cgic_stream_t stream);
int cgic_decode_stream(const cgic_table *t, const uint8_t *in, int64_t nbytes, int64_t *syms,
                       int64_t cap, int64_t *count, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * G. CGIC.compress glue, batched -- CGIC/models/model.py:217-260 (encode side)
 * and :269-397 (decode side).  Bit-identical to looping the reference over
 * the batch at B=1.
 *
 * cgic_compress_streams:
 *   ind     device [B, h, w] int64   (VQ indices on the 1/4-resolution grid)
 *   mask_c  device [B, h/4, w/4], mask_m [B, h/2, w/2], mask_f [B, h, w] int32
 *   mode    0..6 (cgic_router_mode)
 *   out     device [B, 5, slot] uint8, slot = cgic_compress_slot_bytes(t, h, w)
 *   nbytes  device [B, 5] int32: length of each stream; -1 = the mode does not
 *           write that stream (model.py:225-260); 0 = written but empty file;
 *           <= -10 = (CGIC_ERR_* - 10) for that stream (a symbol outside the
 *           table -- KeyError in the reference -- or slot too small)
 *   hist    device [n_symbols] int64 or NULL: += occurrences of every index of
 *           ind (all B*h*w of them) -- the usage counter of quantize.py:79-81,
 *           taken in the same launch
 *   Streams are produced by: masked select in row-major order of each
 *   granularity's own grid (ind[:, ::4, ::4][mask_c==1] ..., :219-221),
 *   Huffman coding with `t`, 1-bit packing of mask_c / mask_m (:230-231).
 *
 * cgic_decompress_streams: inverse (model.py:269-397)
 *   in / nbytes as produced above (device)
 *   ind_out device [B, h, w] int64; mask_*_out device int32 (any may be NULL)
 *   codebook device [K, 4] + z_q device [B, 4, h, w] fp32: optional fused
 *           embedding gather (model.py:391-392), exact codebook rows
 *   codebook2 device [K, 4] + z_q2 device [B, 4, h, w] fp32: optional second gather of the same
 *           indices from another table -- post_quant_conv(codebook) gives post_quant_conv(quant)
 *           (CGIC.decode needs both, model.py:114-116) without a pass over the latent
 *   status  device [B] int32: 0, or CGIC_ERR_INVALID for an image whose streams
 *           the reference would refuse: a stream's symbol count does not match
 *           its mask (more symbols than the grid has cells included), a mask
 *           stream is not exactly 2 + n/8 bytes with pad 8 - n%8 (an empty one
 *           included), or -- only when z_q / z_q2 is asked for: the codebook is the
 *           range the indices are held to -- an index is outside the codebook.
 *           Stricter than the reference in three cases, all CGIC_ERR_INVALID: a
 *           non-canonical mask header (pad + 8 and one more byte), mode 0 with a
 *           cell both coarse and medium (the reference sums -1 there), and an index
 *           stream of one symbol under a mask with another number of cells (the
 *           reference broadcasts it).  The other images of the batch are exact.
 *           What the reference accepts otherwise is accepted with its result: any
 *           pad count 0..255, trailing bytes under the pad, trailing bits that
 *           complete no codeword, an empty coarse / medium index file (all zeros).
 *   nbytes  on the decode side: every stream must satisfy nbytes + 8 <= slot (a
 *           longer one is a read outside the slot: the caller's error).  -1 on a
 *           stream the mode writes: an index stream is read as an EMPTY FILE
 *           (coarse / medium: all zeros; fine: refused where the mask has fine
 *           cells), a mask stream is CGIC_ERR_INVALID in status.  The Python layer
 *           does not get there: CompressedBatch.from_host and container.load raise
 *           ValueError for an absent stream (the reference: FileNotFoundError).
 * ------------------------------------------------------------------------- */
size_t cgic_compress_slot_bytes(const cgic_table *t, int64_t h, int64_t w);
size_t cgic_compress_workspace_bytes(int64_t B, int64_t h, int64_t w);
int cgic_mode_streams(int mode); /* bit i set = stream i is written in this mode */
int cgic_compress_streams(const cgic_table *t, const int64_t *ind, const int32_t *mask_c,
                          const int32_t *mask_m, const int32_t *mask_f, int64_t B, int64_t h,
                          int64_t w, int mode, uint8_t *out, int64_t slot, int32_t *nbytes,
                          int64_t *hist, void *workspace, cgic_stream_t stream);
size_t cgic_decompress_workspace_bytes(int64_t B, int64_t h, int64_t w);
/* Which prefix decoder cgic_decompress_streams launches (same results either way; process-wide, read at launch / capture):
 *   CGIC_DECODE_LATENCY     the split-stream decoders: every 64-bit chunk's exit offset for all 64 entry offsets, composed
 *                           across workgroups -- 1-24 workgroups of 1024 threads and 132 KB of LDS per image; shortest time for
 *                           ONE batch on an otherwise idle GPU (B=64 of 256x256: 15 us).  Small launches (every workgroup of the
 *                           decoder and of the merge on a CU of its own: B <= 32 images of 256x256, a few 768x768 tiles) go out
 *                           as ONE launch: the merge workgroups ride behind the decoder's, build their bitsets and prefixes while
 *                           it runs and pick the symbols up through a per-image ticket (B=1: 23.9 -> 20.8 us per call, one
 *                           768x768 tile 36.7 -> 28.6 us).  Workgroups of this mode wait for workgroups of their own launch
 *                           (the decoder's parts for each other, the merge bands for the decoder): meant for ONE stream of
 *                           launches at a time -- several streams decoding concurrently take CGIC_DECODE_THROUGHPUT, whose
 *                           workgroups never wait for another one
 *   CGIC_DECODE_THROUGHPUT  the self-synchronising decoder: one workgroup per image guesses entry offsets and re-walks until
 *                           they agree -- 256 threads and 41 KB of LDS per 256x256 image, 25 us alone, but it leaves the GPU
 *                           to the kernels of other batches in flight (pipeline.LaneStream: 86 -> 101 GPixel/s); the merge
 *                           that follows runs one band of 1024 threads per image instead of four of 512 (half the instructions)
 *   CGIC_DECODE_AUTO        (default) the same kernels as CGIC_DECODE_LATENCY, but the ONE-launch decoder + merge (whose merge bands
 *                           spin on the decoder workgroups of their own launch) only for launches of at most half the chip's
 *                           workgroups: four such launches in flight on four hardware queues are then resident together and
 *                           no band can be left spinning on a decoder that has no CU yet.  CGIC_DECODE_LATENCY is the
 *                           caller's statement that the call has the GPU to itself: it takes the one-launch form up to the
 *                           whole chip
 * Tables with codes longer than 64 bits and grids whose worst case exceeds the LDS budget always take the split-stream
 * / serial paths.  Returns the previous mode, or CGIC_ERR_INVALID. */
#define CGIC_DECODE_AUTO 0
#define CGIC_DECODE_LATENCY 1
#define CGIC_DECODE_THROUGHPUT 2
int cgic_set_decode_mode(int mode);
/* Telemetry of the self-synchronising decoder (CGIC_DECODE_THROUGHPUT): launches enqueued (or captured) after this call add to
 * device_counters[0..2] (uint32, device memory, zeroed by the caller): [0] fix-point sweeps summed over the images, [1] images,
 * [2] the most sweeps one image needed.  NULL switches it off (the default).  Process-wide; results never depend on it. */
int cgic_decode_stats(unsigned int *device_counters);
int cgic_decompress_streams(const cgic_table *t, const uint8_t *in, int64_t slot, const int32_t *nbytes,
                            int64_t B, int64_t h, int64_t w, int mode, int64_t *ind_out,
                            int32_t *mask_c_out, int32_t *mask_m_out, int32_t *mask_f_out,
                            const float *codebook, int K, int e_dim, float *z_q, const float *codebook2,
                            float *z_q2, int32_t *status, void *workspace, int decoder, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * Three-grain latent merge in front of the quantiser --
 * CGIC/modules/vqvae/vqvae_blocks.py:361-366:
 *   h = up4(h_coarse)*up4(mask0) + up2(h_medium)*up2(mask1) + h_fine*mask2
 *   h_coarse device [B,C,h/4,w/4], h_medium [B,C,h/2,w/2], h_fine [B,C,h,w] fp32
 *   mask_c/m/f device int32 [B,h/4,w/4] / [B,h/2,w/2] / [B,h,w] (the router's)
 *   out device [B,C,h,w] fp32 -- same products, same left-to-right sums: bit-identical
 * Pointers: see the decoder-side calls below (aligned to 4 bytes; out overlaps no input).
 * ------------------------------------------------------------------------- */
int cgic_grain_merge_f32(const float *h_coarse, const float *h_medium, const float *h_fine,
                         const int32_t *mask_c, const int32_t *mask_m, const int32_t *mask_f, int64_t B,
                         int C, int64_t h, int64_t w, float *out, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * Decoder-side masked blends and the two average pools in front of them --
 * CGIC/modules/vqvae/decoder.py:304-305 (AvgPool2d(4,4,0) / AvgPool2d(2,2,0)), :366-367 (applied to the
 * coarse / medium branch), :372-374 and :375-378 (inside the up path):
 *   medium grid:  h = h * up2(mask0) + h_medium * mask1
 *   fine grid:    h = h * up4(mask0) + h * up2(mask1) + h_fine * mask2
 *   h, h_medium / h_fine, out   device [B,C,hh,ww] fp32 on the grid of the call (out may be h itself: in place)
 *   mask_c / mask_m / mask_f    device int32 [B,·,·] at 1/4, 1/2, 1/1 of the FINE grid (the router's / the decoded ones)
 *   same products, same left-to-right sums as the reference expressions: bit-identical.
 * cgic_avgpool_f32: x [planes,H,W] -> out [planes,H/k,W/k], k in {2,4}; row-major running sum of the window
 *   divided by k*k (the order of ATen's CPU kernel: bit-identical to the CPU reference).
 * Pointers of the four _f32 calls (cgic_grain_merge_f32 above, cgic_avgpool_f32, cgic_decoder_blend_medium_f32 / _fine_f32; they share
 * the _h calls' kernels and launch plan, csrc/cgic_merge_plan.h, and so their rules):
 *   - every pointer must be aligned to its 4-byte element: CGIC_ERR_INVALID otherwise (it used to be dereferenced);
 *   - a thread takes 4 consecutive x with 16-byte accesses (the pools: one output from k-element row loads) where the row width and
 *     every pointer's alignment allow; a pointer aligned to 4 or 8 bytes only (a view at a storage offset) gets 1 or 2 x per thread
 *     (the pools: element-wise loads) instead of misaligned wide accesses -- the same bits;
 *   - out == h is the blends' in-place form; ANY other overlap of out with an input (out on h_medium / h_fine or on a mask, out
 *     partly inside h, the merge's or the pool's out on an input) is CGIC_ERR_INVALID -- such calls used to compute wrong values
 *     silently, or to work by accident.
 * Every check precedes the one launch; not available inside a launch group.
 * ------------------------------------------------------------------------- */
int cgic_avgpool_f32(const float *x, int64_t planes, int64_t H, int64_t W, int k, float *out, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * Tiling driver: pad + crop of inference_high_resolution.py as ONE pass (ABI 6).  The script pads the image to a multiple of 16
 * with centred zeros (:145-173, :227-228) and crops the padded image tile by tile (:112-125, :236-244); here every tile of every
 * image is written straight from the unpadded image (zeros where a tile reaches into the pad), one launch for all tiles.
 *   x       device fp32 [N,3,H,W], or with is_u8 the uint8 frames [N,H,W,3]
 *   tiles   host [ntiles] (<= 96): dst = device address of the tile of image 0 -- fp32 [3,th,tw] (16-byte aligned) or uint8
 *           [th,tw,3] (4-byte aligned); image_stride = elements from there to the same tile of the next image; (y0, x0) = the
 *           tile's origin in UNPADDED coordinates (negative inside the pad); th, tw with tw % 4 == 0
 * ------------------------------------------------------------------------- */
typedef struct cgic_tile {
    void *dst;
    int64_t image_stride;
    int y0, x0, th, tw;
} cgic_tile;
int cgic_cut_tiles(const void *x, int is_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_tile *tiles,
                   cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * Tiling driver, the way out (ABI 13): blend + normalise + clamp + unpad of inference_high_resolution.py:231-255 -- and the uint8
 * conversion of write_images (:95-110, inference.py:163-164) -- as ONE launch for all tiles of all N images.  The script
 * accumulates `decoded_tile * gaussian_weights` into a float32 image and the weights into a second one, divides, clamps and
 * slices the pad off.  Its tiles never overlap, so every padded pixel belongs to exactly one tile and the loop is, per value p,
 *     w   = wy[r] * wx[c]                 (float64 product, rounded once)
 *     acc = (float)((double)p * w)        (float32 += float32 * float64 onto 0: computed in double, rounded once to float)
 *     con = (float)w
 *     out = clamp(acc / con, 0, 1)        (IEEE float32 divide)
 *     u8  = (uint8) trunc(255.0f * out)   (float32 product, truncation)
 * which is what the kernel evaluates: bit-identical to the loop on the CPU (the weights do NOT cancel: acc / con differs from p
 * in about one value of five).  con is neither zero nor subnormal for tile extents 16 .. 768.
 *
 * cgic_tile_weights_host: host only, no device work.  The reference's one-dimensional factors (_gaussian_weights, :127-143)
 *   of a tile extent n into out[n]: axis 0 = x (midpoint (n - 1) / 2), axis 1 = y (midpoint n / 2; the asymmetry is the
 *   reference's), exp(-(x - mid) * (x - mid) / (n * n) / (2 * var)) / sqrt(2 * pi * var), var = 0.01, evaluated in the order
 *   of the Python expression with libm's exp: bit-equal to the Python list in the same process.
 *
 * cgic_paste_tiles
 *   tiles    host [ntiles] (1 .. 96): src = device address of the tile of image 0, fp32 [3,th,tw], 16-byte aligned;
 *            image_stride = elements from there to the same tile of the next image (a multiple of 4, below 2^34);
 *            wx [tw], wy [th] = device float64 factors (8-byte aligned), or BOTH NULL: no weighting, out = clamp(p, 0, 1);
 *            (y0, x0) = the tile's origin in UNPADDED coordinates (negative inside the pad); th, tw in 1 .. 65535, tw % 4 == 0
 *   out_f32  device [N,3,H,W] or NULL;  out_u8  device [N,H,W,3] or NULL; at least one of them
 * Every pixel of a tile inside [0,H) x [0,W) is written; tile pixels inside the pad are dropped (the unpad of :255).  Pixels
 * of the outputs that NO tile covers are left untouched.  The tiles, clipped to the image, must be pairwise disjoint
 * (CGIC_ERR_UNSUPPORTED otherwise: the reference's grid never overlaps, and the closed form holds for one tile per pixel).
 * NaN stays NaN in the fp32 output and becomes 0 in the uint8 output (numpy leaves a NaN -> uint8 cast unspecified; this is
 * a definition, not the reference's); +inf -> 1 / 255, -inf -> 0.  N <= 65535.  All checks precede the launch; not available
 * inside a launch group.
 * ------------------------------------------------------------------------- */
int cgic_tile_weights_host(int n, int axis, double *out);
typedef struct cgic_paste_tile {
    const float *src;
    int64_t image_stride;
    const double *wx, *wy;
    int y0, x0, th, tw;
} cgic_paste_tile;
int cgic_paste_tiles(int64_t N, int64_t H, int64_t W, int ntiles, const cgic_paste_tile *tiles, float *out_f32,
                     unsigned char *out_u8, cgic_stream_t stream);
/* ---------------------------------------------------------------------------
 * Partition map (ABI 14): the picture of where the router spent coarse, medium and fine codes -- draw_triple_grain_256res
 * (CGIC/modules/draw.py:78-119; called from model.py:213-214, log_images :421, inference.py -w :148-166 and promised by
 * inference_high_resolution.py:188-189) -- for a batch or for all tiles of N tiled images as ONE launch.  The reference draws it
 * with three nested Python loops and two strided slice assignments per cell (5376 cells per 256x256 image).  Per pixel the loops
 * are a select.  With (gh, gw) the index grid of a tile of th x tw pixels, sh = th / gh, sw = tw / gw (integer divisions) and
 * (y, x) the pixel's position inside the tile, the pixel of EVERY channel becomes a line pixel when any of these holds:
 *     coarse (whatever the indices hold):  y < 4 sh (gh / 4)  and  x < 4 sw (gw / 4)  and  (y % (4 sh) == 0  or  x % (4 sw) == 0)
 *     medium:  y < 2 sh (gh / 2)  and  x < 2 sw (gw / 2)  and  indices[2 (y / (2 sh)), 2 (x / (2 sw))] == 1   (the top-left cell of
 *              the 2x2 block only)  and  (y % (2 sh) == 0  or  x % (2 sw) == 0)
 *     fine:    y < sh gh  and  x < sw gw  and  indices[y / sh, x / sw] == 2  and  (y % sh == 0  or  x % sw == 0)
 * and keeps the source value otherwise: bit-identical to the loops (tests/golden/partition.npz holds the reference's pictures).
 *
 *   src      device, the UNPADDED images: fp32 [N,3,H,W] (4-byte aligned), or with src_u8 the uint8 frames [N,H,W,3]
 *   out_f32  device [N,3,H,W] or NULL;  out_u8  device [N,H,W,3] or NULL; at least one of them.  An output may BE src (the same
 *            address and the same layout: an in-place draw, what the reference does); any other overlap of an output with src, or
 *            of the two outputs, is refused
 *   tiles    host [ntiles] (1 .. 84: what fits a 4 KB kernel-argument block next to the header; callers split larger sets):
 *            every tile in ONE of two forms, the same for all tiles of a call
 *              masks:    mask_c / mask_m / mask_f = device int32 (4-byte aligned), the router's masks of this tile of image 0:
 *                        [th/16,tw/16], [th/8,tw/8], [th/4,tw/4]; th % 16 == tw % 16 == 0; the index grid is (th/4, tw/4) (gh, gw
 *                        must be that or 0) and a cell's index is the FIRST maximum over (up4(mask_c), up2(mask_m), mask_f) with a
 *                        nonzero element counting as 1 -- coarse -> 0, else medium -> 1, else fine -> 2, all zero -> 0: what the
 *                        comment at vqvae_blocks.py:358 means and what argmax gives
 *              indices:  indices = device int64 [gh,gw] (8-byte aligned) of this tile of image 0, the reference function's own
 *                        argument, any values (only == 1 and == 2 matter); gh, gw >= 1 with th / gh >= 1 and tw / gw >= 1
 *                        (CGIC_ERR_UNSUPPORTED otherwise); the three masks NULL
 *            image_stride_tiles = tiles between this tile of image n and of image n + 1 (T of its shape group in an image-major
 *            batch, 1 for a plain batch; 0 .. 2^31 - 1): each array advances by that many of its OWN tile sizes;
 *            (y0, x0) = the tile's origin in UNPADDED image coordinates (negative inside the pad); th, tw in 1 .. 65535
 * A line pixel is -1.0f in the fp32 output and 1 in the uint8 output: 1 is the wrap numpy performs on x86-64 for write_images'
 * conversion (255 * -1.0f).astype(uint8) (inference_high_resolution.py:103; numpy leaves the cast of a negative float
 * unspecified) -- a definition, as NaN -> 0 is for cgic_paste_tiles.  Any other pixel is the source value: fp32 -> fp32 and
 * uint8 -> uint8 the value itself (trunc(255.0f * (b / 255.0f)) == b for all 256 bytes), fp32 -> uint8
 * trunc(255.0f * clamp(p, 0, 1)) with NaN -> 0 (as cgic_paste_tiles), uint8 -> fp32 b / 255.0f (IEEE divide: T.ToTensor()).
 * Tile pixels inside the pad are dropped; output pixels NO tile covers are left untouched.  The tiles, clipped to the image, must
 * be pairwise disjoint (CGIC_ERR_UNSUPPORTED).  N <= 65535; H, W in 1 .. 65535.  All checks precede the launch; not available
 * inside a launch group.
 * ------------------------------------------------------------------------- */
typedef struct cgic_partition_tile {
    const int32_t *mask_c, *mask_m, *mask_f;
    const int64_t *indices;
    int64_t image_stride_tiles;
    int y0, x0, th, tw, gh, gw;
} cgic_partition_tile;
int cgic_partition_map(const void *src, int src_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_partition_tile *tiles,
                       float *out_f32, unsigned char *out_u8, cgic_stream_t stream);
/* cgic_cut_tiles for the tiles of ONE shape + cgic_entropy_maps_f32 / _u8 on them, in one pass: a lane of the map kernel reads its pixels
 * from the source window (zeros inside the pad) and the tile batch is written as a by-product -- 12 B read + 12 B written per pixel
 * instead of 12 + 12 for the cut and 12 again for the maps.  Recorded like the other entropy calls inside a launch group.
 *   src      device fp32 [N,3,H,W] (unpadded), or with is_u8 the uint8 frames [N,H,W,3]
 *   origins  host [T][2] int: (y0, x0) of the T (<= 48) tiles of this shape in unpadded coordinates; the batch is image-major:
 *            tile b of the outputs = (image b / T, tile b % T)
 *   x_out    device fp32 [N*T, 3, th, tw]: the tiles (from frames: byte / 255 as T.ToTensor() rounds it) -- required: it is what the
 *            conv encoder and the router's refinement (cgic_pixels.x, is_u8 = 0) read
 *   e8, e16, flat8 as cgic_entropy_maps_f32 for a batch of N*T images of th x tw; bit-identical to the two separate calls. */
int cgic_entropy_maps_tiles(const void *src, int is_u8, int64_t N, int64_t H, int64_t W, int T, const int *origins,
                            int64_t th, int64_t tw, const float *bins, int nbins, float sigma, float *x_out,
                            float *e8, float *e16, float *flat8, cgic_stream_t stream);
int cgic_decoder_blend_medium_f32(const float *h, const float *h_medium, const int32_t *mask_c, const int32_t *mask_m,
                                  int64_t B, int C, int64_t hh, int64_t ww, float *out, cgic_stream_t stream);
int cgic_decoder_blend_fine_f32(const float *h, const float *h_fine, const int32_t *mask_c, const int32_t *mask_m,
                                const int32_t *mask_f, int64_t B, int C, int64_t hh, int64_t ww, float *out,
                                cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * The merge, the pools and the blends on half-precision features (ABI 16): what the reference computes when its conv
 * nets run under torch.autocast in fp16 or bf16.  There `h * upsample(mask.float()) + own * mask` promotes to fp32 and
 * AvgPool2d keeps the half type, so:
 *   in_dtype   CGIC_DT_F16 or CGIC_DT_BF16: the type of EVERY feature tensor of the call (CGIC_DT_F32 is
 *              CGIC_ERR_UNSUPPORTED: that is the _f32 entry point's)
 *   out_dtype  CGIC_DT_F32 (the reference's promotion for the merge and the blends) or in_dtype (AvgPool2d's result; for the
 *              merge and the blends an option the reference does not have: its fp32 value rounded once)
 * Arithmetic: the features are upcast exactly (fp16 subnormals included), the products, the left-to-right sums and the
 * pool's row-major running sum / (float)(k*k) are the fp32 operations of the _f32 kernels, a half output is rounded once to
 * nearest-even (fp16 overflow: +-Inf).  Bit-identical to the reference's expression on the CPU.  Products and sums, not
 * selects: an Inf or NaN under a zero mask is a NaN.
 * Shapes, masks and kernels as the _f32 siblings (one kernel family, one plan).  A pointer must be aligned to its own element; wider alignment and a row width
 * that is a multiple of 8 let a thread take 8 consecutive x with 16-byte accesses, otherwise 4, 2 or 1 (csrc/cgic_merge_plan.h).
 * `out` may be `h` itself for the two blends when out_dtype == in_dtype (in place); any other overlap of `out` with an input
 * is CGIC_ERR_INVALID.  Every check precedes the one launch; not available inside a launch group.
 *   cgic_grain_merge_h            vqvae_blocks.py:361-366
 *   cgic_avgpool_h                decoder.py:304-305,366-367
 *   cgic_decoder_blend_medium_h   decoder.py:372-374
 *   cgic_decoder_blend_fine_h     decoder.py:375-378
 * ------------------------------------------------------------------------- */
#define CGIC_DT_F32 0
#define CGIC_DT_F16 1
#define CGIC_DT_BF16 2
int cgic_grain_merge_h(const void *h_coarse, const void *h_medium, const void *h_fine, int in_dtype, const int32_t *mask_c,
                       const int32_t *mask_m, const int32_t *mask_f, int64_t B, int C, int64_t h, int64_t w, void *out,
                       int out_dtype, cgic_stream_t stream);
int cgic_avgpool_h(const void *x, int in_dtype, int64_t planes, int64_t H, int64_t W, int k, void *out, int out_dtype,
                   cgic_stream_t stream);
int cgic_decoder_blend_medium_h(const void *h, const void *h_medium, int in_dtype, const int32_t *mask_c, const int32_t *mask_m,
                                int64_t B, int C, int64_t hh, int64_t ww, void *out, int out_dtype, cgic_stream_t stream);
int cgic_decoder_blend_fine_h(const void *h, const void *h_fine, int in_dtype, const int32_t *mask_c, const int32_t *mask_m,
                              const int32_t *mask_f, int64_t B, int C, int64_t hh, int64_t ww, void *out, int out_dtype,
                              cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * The decoder's SpatialNorm (ABI 17) -- CGIC/modules/vqvae/decoder.py:34-53, and on request the swish behind it (:29-31):
 *     zq = interpolate(zq, size=f.shape[-2:], mode="nearest");  new_f = GroupNorm(groups, eps, affine)(f) * conv_y(zq) + conv_b(zq)
 * as one pass over the features (csrc/cgic_norm.hip; every check and the launch plan: csrc/cgic_norm_plan.h).
 *   f          device [B, C, H, W] of in_dtype (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16), contiguous
 *   zq         device [B, 4, hq, wq] fp32.  Each axis at an integer ratio of the features', up-sampled (H % hq == 0: source row
 *              y / (H / hq)) or sub-sampled (hq % H == 0: source row y * (hq / H)), the two axes independently: torch's "nearest" at
 *              these ratios.  Any other ratio is CGIC_ERR_UNSUPPORTED.
 *   groups, eps, gn_weight, gn_bias    the GroupNorm: C % groups == 0; weight and bias device fp32 [C]
 *   wy, by, wb, bb    conv_y and conv_b: device fp32 [C, 4] (the 1x1 conv weight's own memory) and [C]
 *   swish      != 0: x * sigmoid(x) of the result, as v / (1 + exp(-v))
 *   out        device [B, C, H, W] of out_dtype: CGIC_DT_F32, or in_dtype (the fp32 value rounded once to nearest-even).  May be f
 *              itself when the types are equal (in place); any other overlap of out with an input is CGIC_ERR_INVALID.
 *   workspace  device, cgic_spatial_norm_workspace_bytes(...) bytes, 8-byte aligned (NULL where that is 0)
 * Values: mean and biased variance of a group in float64 about the group's first element, each of mean and rstd rounded once to
 * fp32; then per element in fp32, without contraction: n = ((x - mean) * rstd) * gamma + beta, y = by + sum_k wy[k] * zq_k (k in
 * order), b likewise, v = n * y + b.  A NaN or Inf anywhere in a group makes that group's output NaN throughout, as in the reference.
 * Deterministic: one launch (one workgroup per group) where a group fits a workgroup's LDS budget and the batch has groups enough
 * to fill the chip, otherwise two launches ordered by the stream whose partial sums are added in a fixed order.
 * cgic_spatial_norm_one_launch says which: 1, 0, or CGIC_ERR_* for a shape the call refuses.  A pointer must be aligned to its own
 * element; wider alignment and a row width that is a multiple of 8 (fp32: 4) give 16-byte accesses.  Every check precedes the
 * first launch; not available inside a launch group.
 * ------------------------------------------------------------------------- */
int cgic_spatial_norm(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, const float *zq, int64_t hq, int64_t wq,
                      int groups, double eps, const float *gn_weight, const float *gn_bias, const float *wy, const float *by,
                      const float *wb, const float *bb, int swish, void *out, int out_dtype, void *workspace,
                      size_t workspace_bytes, cgic_stream_t stream);
size_t cgic_spatial_norm_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups);
int cgic_spatial_norm_one_launch(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups);

/* ---------------------------------------------------------------------------
 * SpatialNorm for training (ABI 19): the forward that keeps the groups' statistics, and the backward.
 *
 * cgic_spatial_norm_train is cgic_spatial_norm (same arguments, same checks, same kernels, the same bits in `out`) that also writes
 *   stats      device fp32 [B * groups][2] = (mean, rstd) of each group, as the forward rounded them; a tensor of its own.
 *
 * cgic_spatial_norm_backward, with go the gradient of the forward's result:
 *   f, zq, the six parameters, groups, swish: what the forward was given; stats: what it wrote.
 *   go         device [B, C, H, W] of go_dtype: CGIC_DT_F32, or in_dtype
 *   df         device [B, C, H, W] of df_dtype: CGIC_DT_F32, or in_dtype (the fp32 value rounded once).  May be go itself when the
 *              types are equal; an output overlaps nothing else.
 *   dzq        device fp32 [B, 4, hq, wq]; an element that a sub-sampled axis never reads gets exactly 0
 *   dgn_weight, dgn_bias, dby, dbb   device fp32 [C];   dwy, dwb   device fp32 [C, 4]
 *   Every output may be NULL: it is not computed (without dzq no dz partials; without dwy, dby, dwb and dbb two plane sums per
 *   channel instead of twelve; without df no apply launch).  At least one is wanted.
 *   workspace  device, cgic_spatial_norm_backward_workspace_bytes(...) bytes (a function of the shape alone), 16-byte aligned.  It
 *              need not be zeroed: the call writes every partial it reads.
 * Values: per element in fp32 with the forward's mean and rstd, the pre-activation v recomputed, not stored; every sum in float64.
 * Three launches ordered by the stream (cgic_norm_bwd_plan.h), no atomics, no host synchronisation, no allocation: two calls give
 * the same bits, df and dzq of an image do not depend on its batch, and the chain can be captured in a graph.  A NaN in f makes the
 * gradients NaN where the reference's are; +-Inf in f or go is not specified (torch's own GroupNorm backward uses another algebra
 * there).  Every check precedes the first launch; not available inside a launch group.
 * ------------------------------------------------------------------------- */
int cgic_spatial_norm_train(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, const float *zq, int64_t hq, int64_t wq,
                            int groups, double eps, const float *gn_weight, const float *gn_bias, const float *wy, const float *by,
                            const float *wb, const float *bb, int swish, void *out, int out_dtype, float *stats, void *workspace,
                            size_t workspace_bytes, cgic_stream_t stream);
int cgic_spatial_norm_backward(const void *f, int in_dtype, const void *go, int go_dtype, int64_t B, int C, int64_t H, int64_t W,
                               const float *zq, int64_t hq, int64_t wq, int groups, const float *stats, const float *gn_weight,
                               const float *gn_bias, const float *wy, const float *by, const float *wb, const float *bb, int swish,
                               void *df, int df_dtype, float *dzq, float *dgn_weight, float *dgn_bias, float *dwy, float *dby,
                               float *dwb, float *dbb, void *workspace, size_t workspace_bytes, cgic_stream_t stream);
size_t cgic_spatial_norm_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups);

/* ---------------------------------------------------------------------------
 * The encoder's GroupNorm (ABI 21) -- CGIC/modules/vqvae/vqvae_blocks.py:34, GroupNorm(groups, eps, affine), and on request the swish
 * that ResnetBlock and the norm_out heads put behind it: the kernels above instantiated without zq (no zq, y or b value is loaded
 * or multiplied), for inference and for training.
 *   f, groups, eps, gn_weight, gn_bias, swish, out, workspace: as cgic_spatial_norm's; the workspace is sized by
 *   cgic_spatial_norm_workspace_bytes and the form answered by cgic_spatial_norm_one_launch (both depend on the shape alone).
 * Values: the same statistics; per element in fp32, without contraction: v = ((x - mean) * rstd) * gamma + beta, with swish
 * v / (1 + exp(-v)).  On finite inputs this is bit for bit cgic_spatial_norm with wy = wb = 0, by = 1, bb = 0.
 * cgic_group_norm_train also writes stats [B * groups][2] = (mean, rstd); its out is cgic_group_norm's bit for bit.
 * cgic_group_norm_backward: df, dgn_weight (sum go' * xhat) and dgn_bias (sum go'), each optional (NULL), at least one wanted; go' is
 * go, with swish go times the swish's derivative at the recomputed v.  The same three launches (reduce, finish, apply) with two
 * float64 plane sums per channel; no atomics; df may be go itself when the types are equal.  workspace:
 * cgic_group_norm_backward_workspace_bytes(...) bytes, 16-byte aligned, need not be zeroed.
 * Every check precedes the first launch (the same refusals as the modulated calls, under the names group_norm, group_norm_train
 * and group_norm_backward); not available inside a launch group.
 * ------------------------------------------------------------------------- */
int cgic_group_norm(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups, double eps, const float *gn_weight,
                    const float *gn_bias, int swish, void *out, int out_dtype, void *workspace, size_t workspace_bytes, cgic_stream_t stream);
int cgic_group_norm_train(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups, double eps, const float *gn_weight,
                          const float *gn_bias, int swish, void *out, int out_dtype, float *stats, void *workspace, size_t workspace_bytes,
                          cgic_stream_t stream);
int cgic_group_norm_backward(const void *f, int in_dtype, const void *go, int go_dtype, int64_t B, int C, int64_t H, int64_t W, int groups,
                             const float *stats, const float *gn_weight, const float *gn_bias, int swish, void *df, int df_dtype,
                             float *dgn_weight, float *dgn_bias, void *workspace, size_t workspace_bytes, cgic_stream_t stream);
size_t cgic_group_norm_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups);

/* ---------------------------------------------------------------------------
 * AttnBlock's attention (ABI 18) -- CGIC/modules/vqvae/decoder.py:189-213, vqvae_blocks.py:168-193:
 *     w = softmax_j(scale * sum_c q[c,i] k[c,j]);   out[c,i] = sum_j v[c,j] w[i,j]
 * one head as wide as the channel count, computed flash-style: no tokens x tokens tensor is ever written to memory
 * (csrc/cgic_attn.hip; every check and the launch plan: csrc/cgic_attn_plan.h).
 *   q, k, v    device, [C, N] per image with the tokens contiguous (what the 1x1 convs return), of in_dtype (CGIC_DT_F32,
 *              CGIC_DT_F16 or CGIC_DT_BF16); image b begins b * {q,k,v}_batch_stride ELEMENTS behind the pointer (>= C * N; C * N when
 *              dense), so the three thirds of one [B, 3C, N] qkv tensor can be passed as they lie
 *   C          256 or 512 (the model's widths); any other width is CGIC_ERR_UNSUPPORTED.  N >= 1, a multiple of nothing.
 *   scale      finite, >= 0; the reference passes int(C) ** -0.5.  0, or a scale whose product with log2(e) rounds to 0 in fp32, gives
 *              uniform weights: out is the mean of v, lse is ln N
 *   out        device [B, C, N] dense of out_dtype: in_dtype, or CGIC_DT_F32.  A half out is the fp32 result rounded once to
 *              nearest-even.
 *   lse        device fp32 [B, N], or NULL: ln sum_j exp(scale * s_ij) (cgic_attention_backward reads it), as max * scale + ln(row sum) in
 *              float64 from the fp32 maximum and row sum, rounded once
 *   workspace  cgic_attention_workspace_bytes(...) bytes; that is 0 for every shape (keys are never split over workgroups), NULL is fine
 * Values: the scores, the running maximum, the row sum and the accumulator are fp32.  fp32 inputs are multiplied as fp32
 * (v_mfma_f32_32x32x2_f32), never as a half type; fp16 / bf16 inputs on v_mfma_f32_32x32x16_{f16,bf16}, the weights p rounded once
 * to the half type in front of the second product -- as torch's half bmm takes them -- while the row sum adds the unrounded p.
 * NaN: one in q[:, i] makes query i NaN, one in k the whole image, one in v[c, :] channel c -- the reference's pattern.
 * Infinite scores (an Inf in q or k), as softmax over the whole row has them: a key whose score is -inf weighs 0, wherever it lies
 * -- also when every key of the leading tiles scores -inf --, and the query is finite if any other key is; a query with a +inf
 * score, with scores of both signs of inf, or whose every key scores -inf is NaN at every channel; with scale 0 an infinite score is
 * inf * 0 = NaN.  Finite scores saturate nothing: the maximum is subtracted, so a common offset of thousands changes no weight.
 * Infinite v: out[c, i] is v[c, :] weighed as IEEE sums do -- +Inf (-Inf) where channel c holds infinities of one sign at keys of
 * non-zero weight, NaN where it holds both signs, or an infinity at a key whose weight is taken as 0 (0 * inf).
 * A weight below 2^-64 of the row's largest is taken as exactly 0; a row whose other weights are all below that returns v's own
 * column of the winning key bit for bit, in the fp32 out as in a half out.
 * lse on such rows: where ln sum_j exp(scale * s_ij) and the row's softmax weights are finite -- v plays no part -- lse is that number
 * (a -inf score adds 0 to the sum); on every other row it is non-finite: NaN for a NaN or +inf score, -inf where every key scores -inf.
 * Deterministic: an image's bits depend on its own q, k, v alone (not on B, not on scheduling); no atomics, no workgroup waits for
 * another.  out and lse must overlap no input and not each other (CGIC_ERR_INVALID); a pointer must be aligned to its own element;
 * 16-byte aligned v with N % 8 == 0 gets 16-byte loads, anything else element loads.  Every check precedes the one launch, so a
 * refused call enqueues nothing; not available inside a launch group.
 * cgic_attention_supported: 1 if the call is built for these types and this shape, 0 if not (the caller then evaluates the
 * expression some other way), CGIC_ERR_INVALID for arguments that are wrong in themselves.
 * ------------------------------------------------------------------------- */
int cgic_attention(const void *q, const void *k, const void *v, int in_dtype, int64_t B, int C, int64_t N, int64_t q_batch_stride,
                   int64_t k_batch_stride, int64_t v_batch_stride, double scale, void *out, int out_dtype, float *lse, void *workspace,
                   size_t workspace_bytes, cgic_stream_t stream);
size_t cgic_attention_workspace_bytes(int in_dtype, int64_t B, int C, int64_t N);
int cgic_attention_supported(int in_dtype, int out_dtype, int64_t B, int C, int64_t N);

/* ---------------------------------------------------------------------------
 * The attention's backward pass (ABI 20), again with no tokens x tokens tensor in memory (csrc/cgic_attn_bwd.hip; every check and the
 * geometry of the launches: csrc/cgic_attn_bwd_plan.h).  With s_ij = scale * sum_c q[c,i] k[c,j] and go the gradient of the forward's out:
 *     P_ij = exp(s_ij - lse_i)    delta_i = sum_c go[c,i] out[c,i]    dP_ij = sum_c go[c,i] v[c,j]    dS_ij = P_ij (dP_ij - delta_i)
 *     dv[c,j] = sum_i go[c,i] P_ij      dq[c,i] = scale sum_j dS_ij k[c,j]      dk[c,j] = scale sum_i dS_ij q[c,i]
 *   q, k, v, C, N, scale, the three batch strides: what cgic_attention was given (views of one [B, 3C, N] tensor are read where they lie)
 *   go         device, [C, N] per image of in_dtype, image b go_batch_stride ELEMENTS behind the pointer (>= C * N; the four batch
 *              strides are at most 2^59 / B elements: CGIC_ERR_INVALID beyond, so that no extent of the aliasing check can wrap)
 *   out        device [B, C, N] dense of in_dtype: what the forward returned with out_dtype = in_dtype
 *   lse        device fp32 [B, N]: what the forward wrote
 *   dq, dk, dv device [B, C, N] dense of grad_dtype: CGIC_DT_F32, or in_dtype (the fp32 value rounded once to nearest-even).  Each may be
 *              NULL: it is neither computed nor written (without dq no query-owning launch; without dk and dv no key-owning launch,
 *              with one of them half of its products; without dq and dk no delta).  All three NULL: nothing is done, CGIC_OK.
 *   workspace  device, cgic_attention_backward_workspace_bytes(...) bytes -- delta: 4 bytes per token and image, rounded up to 16; a
 *              function of the shape alone --, 16-byte aligned.  It need not be zeroed: the call writes every element it reads.
 * Up to three launches ordered by the stream: delta; a launch whose workgroups own 32 queries and walk the keys (dq); one whose
 * workgroups own 32 keys and walk the queries (dk, dv).  P and dS are recomputed per tile on the chip and all sums are kept in
 * registers.  No atomics, no workgroup waits for another, every sum in a fixed order, no host synchronisation, no allocation: two
 * calls give the same bits, an image's gradients do not depend on its batch, and the chain can be captured in a graph.
 * Values: scores and dP in fp32 from the exactly upcast inputs (fp32 inputs on v_mfma_f32_32x32x2_f32, never through a half type;
 * fp16 / bf16 on v_mfma_f32_32x32x16_{f16,bf16}); P = exp2((s * scale - lse) * log2 e) in fp32, exactly 0 below 2^-64; tail keys and
 * queries 0 by a select; P and dS rounded once to the operand type in front of the second products; delta fp32; scale applied once,
 * in fp32, to the finished sums.  With scale 0, dq and dk are exact zeros.
 * NaN: one in go[c0, i0] reaches dq[:, i0], all of dk and dv[c0, :] of its image; one in q[c0, i0] dq[:, i0] and all of dk and dv; one in
 * k all three; one in v all of dq and dk and nothing of dv -- as float64 autograd of the reference's expression, and never another
 * image.  +-Inf in an input, and rows whose lse is not finite, are not specified.
 * An output must overlap no input, no other output and not the workspace (CGIC_ERR_INVALID); a pointer must be aligned to its own
 * element; rows that begin 16-byte aligned (N % 8 == 0, aligned pointer and stride) get 16-byte loads.  Every check precedes the
 * first launch, so a refused call enqueues nothing; not available inside a launch group.
 * cgic_attention_backward_supported: 1 if the call is built for these types and this shape, 0 if not, CGIC_ERR_INVALID for arguments
 * that are wrong in themselves.
 * ------------------------------------------------------------------------- */
int cgic_attention_backward(const void *go, const void *q, const void *k, const void *v, const void *out, const float *lse, int in_dtype,
                            int64_t B, int C, int64_t N, int64_t go_batch_stride, int64_t q_batch_stride, int64_t k_batch_stride,
                            int64_t v_batch_stride, double scale, void *dq, void *dk, void *dv, int grad_dtype, void *workspace,
                            size_t workspace_bytes, cgic_stream_t stream);
size_t cgic_attention_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t N);
int cgic_attention_backward_supported(int in_dtype, int grad_dtype, int64_t B, int C, int64_t N);

/* embedding gather on its own (model.py:121,391-392): out[b, c, p] = codebook[ind[b, p], c] */
int cgic_embedding_gather_f32(const int64_t *ind, int64_t B, int64_t hw, const float *codebook, int K,
                              int e_dim, float *out, int32_t *status, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * H'. One call per call the reference makes -- CGIC.compress for one image or a batch of images of one size, hot path only
 * (CGIC/models/model.py:206-401 without the conv encoder / decoder; the loop of inference.py:157-166 calls it once per image):
 *   Entropy(8), Entropy(16) on the pixels (model.py:99-101)  ->  [VectorQuantize2.forward + the per-image router, one launch]
 *   (model.py:110-112, vqvae_blocks.py:355)  ->  Huffman / mask coding of the five streams (model.py:217-260)  ->  and, if any
 *   decode output is given, the way back (model.py:269-397): prefix decoder, scatter / merge, codebook gather.
 * Exactly the launches of cgic_entropy_maps_f32 / _u8, cgic_vq_forward_route_f32 (with the threshold-band refinement from these
 * pixels), cgic_compress_streams and cgic_decompress_streams with the same arguments -- bit-identical results -- enqueued by
 * ONE call on `stream`: an eager caller pays one foreign call instead of four (+ their Python around them: B = 1 eager
 * 93 -> the time of the launches themselves).
 *   x        device fp32 [B,3,H,W], or with x_is_u8 the uint8 frames [B,H,W,3]; H, W multiples of 16
 *   z        device fp32 [B,4,H/4,W/4]: the latent behind quant_conv (the conv encoder is the caller's)
 *   e8, e16, flat8   device fp32 [B,H/8,W/8], [B,H/16,W/16], [B,H/8,W/8]: written (the maps are results of the call)
 *   x_out    device fp32 [B,3,H,W] or NULL (x_is_u8 only): ToTensor's output, as cgic_entropy_maps_u8
 *   ind, mask_c/m/f, z_q (or NULL), loss (or NULL), streams [B,5,slot], nbytes [B,5], hist (or NULL): as the single calls
 *   dind ... status: the decode side's outputs (cgic_decompress_streams); dind == NULL: encode only
 *   ws_vq (cgic_vq_workspace_bytes(B*h*w); may be NULL iff loss is), ws_compress (cgic_compress_workspace_bytes),
 *   ws_decompress (cgic_decompress_workspace_bytes; NULL iff dind is), ws_refine (optional: the row bands of large tiles then
 *   split a threshold band between them instead of evaluating it each)
 * ------------------------------------------------------------------------- */
typedef struct cgic_image_io {
    const void *x; int x_is_u8;
    const float *z;
    float *x_out, *e8, *e16, *flat8;
    int64_t *ind; float *z_q, *loss;
    int32_t *mask_c, *mask_m, *mask_f;
    uint8_t *streams; int64_t slot; int32_t *nbytes; int64_t *hist;
    int64_t *dind; int32_t *dmask_c, *dmask_m, *dmask_f; float *dz_q; int32_t *status;
    void *ws_vq, *ws_compress, *ws_decompress;
    void *ws_refine; size_t ws_refine_bytes;     /* cgic_router_refine_scratch_bytes(B, H/16, W/16, 1) bytes or NULL: cgic_pixels.scratch of the call */
} cgic_image_io;
int cgic_compress_image(const cgic_table *t, const float *codebook, int K, int e_dim, const void *prepared, int64_t B, int64_t H,
                        int64_t W, double coarse_ratio, double medium_ratio, float beta, int legacy, const float *bins, int nbins,
                        float sigma, int decoder, const cgic_image_io *io, int *mode_out, cgic_stream_t stream);

/* The same for the tiled driver of high-resolution images (inference_high_resolution.py:112-173 pad + grid, :236-257 the
 * per-tile compress loop): the tiles of N images of one size, grouped by shape (a 2040x1356 image: six tiles of four shapes),
 * through ONE launch chain -- [pad + crop + both entropy maps] -> [VQ + per-tile router] -> stream coder -> (decoder + merge) --
 * every link one launch for all shape groups (launch groups, cgic_group_begin / _launch).  One foreign call per image instead of
 * ~30 recorded ones (eager: 0.54 ms -> the launches themselves).  Per group:
 *   ntiles, th, tw, origins (host [ntiles][2]: (y0, x0) of the tiles in UNPADDED coordinates, may be negative / reach beyond
 *   the image: the centred pad), share (of the chip: the group's pixels / all pixels), and io: the buffers of the group's batch
 *   of N * ntiles tiles (image-major), as cgic_compress_image -- io.x / x_is_u8 are ignored (the tiles come from `src`),
 *   io.x_out (the fp32 tile batch) is REQUIRED, io.z is the latent of the tiles.
 * mode_out: the routing mode (the same for all groups).  At most cgic_group_max() groups. */
typedef struct cgic_tile_group {
    int ntiles, th, tw;
    const int *origins;
    double share;
    cgic_image_io io;
} cgic_tile_group;
int cgic_compress_tiled(const cgic_table *t, const float *codebook, int K, int e_dim, const void *prepared, const void *src,
                        int src_is_u8, int64_t N, int64_t H, int64_t W, int ngroups, const cgic_tile_group *groups,
                        double coarse_ratio, double medium_ratio, float beta, int legacy, const float *bins, int nbins, float sigma,
                        int decoder, int *mode_out, cgic_stream_t stream);

/* ---------------------------------------------------------------------------
 * I. Rate tables (ABI 9), rate curves (ABI 10), rate curves of tiled images (ABI 11) and the device-side rate pick (ABI 12): the .bin sizes CGIC.compress (model.py:217-262) would write for each of C candidate granularity
 * ratios, without writing a stream -- the "which ratio gives which bpp on THIS image" question of a controllable codec.
 *
 * Exactness.  In the encoder's merge h = up4(h_c)*up4(m_c) + up2(h_m)*up2(m_m) + h_f*m_f (vqvae_blocks.py:361-366) every
 * position takes exactly one head's vector (for finite x: x*1 + y*0 + z*0 == x bit for bit); quant_conv is a 1x1 convolution
 * (per position) and the VQ works on one vector at a time.  So ind[:, ::4, ::4] at a coarse position is VQ(quant_conv(h_c))
 * there, likewise ind[:, ::2, ::2] on the medium grid and ind on the fine grid: the VQ of each head at its own resolution
 * (n + n/4 + n/16 vectors) gives the indices of EVERY ratio.  And HuffmanCoding.compress (indices_coding.py:113-124) writes an
 * empty file for an empty list, else nbits // 8 + 2 bytes (one header byte, 1..8 pad bits -- also when nbits % 8 == 0); a mask
 * stream is n // 8 + 2 bytes for its fixed n (mask_coding.py): a stream's size depends on the masks only through the number
 * and the summed code lengths of the symbols they select.  LIMIT: the argument needs finite latents -- inf * 0 is NaN in the
 * reference's merge, so a head holding +-inf or NaN poisons the merged vector at positions that take ANOTHER head.
 *
 * cgic_rate_table:
 *   ind_c / ind_m / ind_f  device int64 [B,h16,w16] / [B,2h16,2w16] / [B,4h16,4w16]: the per-head VQ indices (latent grids
 *            h/4, h/2, h of the [B,4,h,w] latent, h = 4 h16)
 *   e16, e8, B, h16, w16, per_image, refine   exactly what cgic_router_f32 takes (refine->scratch: required when
 *            cgic_router_refine_in_lds(...) == 0, as there)
 *   C, coarse, medium   host [C] candidate ratios, 1 <= C <= 64
 *   nbytes   device int32 [C, B, 5]: nbytes[c, b, s] == nbytes[b, s] of cgic_compress_streams called after cgic_router_f32 at
 *            (coarse[c], medium[c]) with the same per_image / refine, on ind = cgic_gather_grain_indices(.., those masks) --
 *            except that a stream the mode does not write is 0 here (-1 there).  Bytes are per image also when per_image = 0
 *            routes the flattened batch as one segment.  <= -10: a selected symbol outside the table (as cgic_compress_streams).
 *   workspace device, cgic_rate_table_workspace_bytes(...) bytes, 16-byte aligned: the [C, ...] stack of the masks
 * Every candidate is checked (mode, k <= n, the refinement's requirements -- for segments beyond the LDS also the scratch)
 * before anything is enqueued: a bad candidate returns CGIC_ERR_INVALID / _UNSUPPORTED with nothing written.
 * Launches: one router launch for all candidates (grid: the router's workgroups x C) into the mask stack + one reduction (B x C
 * workgroups: code lengths in LDS, DPP wave sums).  Segments whose refinement is the launch chain of cgic_router_f32
 * (cgic_router_refine_in_lds == 0) are routed candidate by candidate through cgic_router_f32, sequentially on `stream`: one
 * scratch-carrying launch in flight at a time.  Not inside a launch group.
 *
 * cgic_gather_grain_indices: ind_out[b,y,x] = mask_f ? ind_f : up2(mask_m) ? up2(ind_m) : up4(ind_c) -- int64 [B,h,w] in one pass;
 *   masks int32 as cgic_router_f32 writes them (a partition of the grid), h % 4 == w % 4 == 0.  Equal to the VQ indices of the
 *   merged latent (finite latents, see above): what cgic_compress_streams takes for the chosen ratio.
 * ------------------------------------------------------------------------- */
size_t cgic_rate_table_workspace_bytes(int64_t B, int64_t h16, int64_t w16, int C, int per_image);
int cgic_rate_table(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                    const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16, int C, const double *coarse,
                    const double *medium, int per_image, const cgic_pixels *refine, int32_t *nbytes, void *workspace,
                    cgic_stream_t stream);
int cgic_gather_grain_indices(const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f, const int32_t *mask_c,
                              const int32_t *mask_m, const int32_t *mask_f, int64_t B, int64_t h, int64_t w, int64_t *ind_out,
                              cgic_stream_t stream);

/* Rate curves (ABI 10): the sizes of EVERY medium rank of one coarse ratio.  With the coarse ratio fixed, the router's medium
 * decision is one integer, the rank K of the medium threshold among the 8x8-patch entropies (RouterTriple.py:28-32): n8 + 1 =
 * 4 h16 w16 + 1 settings per image, of which a rate table samples at most 64.
 *
 * cgic_rate_curve:
 *   t, ind_c / ind_m / ind_f, e16, e8, B, h16, w16   as cgic_rate_table.  The maps may hold ANY float: NaN (what a NaN pixel
 *            makes of its patches), +-Inf, negatives, zeros of either sign, denormals -- every comparison below is the router's
 *            (torch.sort's order with NaN last, float '<', the fp32 product e8 * 0 under a coarse patch)
 *   coarse_ratio  in [0, 1].  > 0: the coarse rank k_c = round(n16 * coarse_ratio) and the stream set of mode 0; == 0: mode 1
 *            (no coarse patch; K = round(n8 * medium))
 *   nbytes   device int32 [B, n8 + 1, 5]: nbytes[b, K, :] == nbytes[c, b, :] of cgic_rate_table with per_image = 1 and
 *            refine = NULL (every image routed on its own thresholds, on the maps AS GIVEN) for a candidate c whose ranks
 *            (cgic_router_ranks) are (k_c, K): the coarse mask is e16 < s16[k_c - 1] (k_c == 0: index 0), the medium list
 *            e8 * (1 - up2(gate_coarse)), its threshold t = sorted[K - 1] (K == 0: index 0), medium = e8 < t and not coarse
 *            (strict: tied patches move together, so the curve has plateaus and is NOT monotone in K), fine = the rest.  All K
 *            in 0 .. n8 are written; which of them a ratio reaches is host arithmetic (cgic_router_ranks).  <= -10: a selected
 *            symbol outside the table, as cgic_rate_table.
 *   workspace device, cgic_rate_curve_workspace_bytes(...) bytes, 16-byte aligned; on return int32 [B, 4] per image: the
 *            number of coarse patches, the coarse threshold's fp32 bit pattern (+-0 as +0, any NaN as 0x7FC00000; 0 when k_c == 0),
 *            the medium / fine code bits of all non-coarse patches
 * One launch, one workgroup per image: the image's patches are sorted ONCE by entropy in LDS (64-bit words: an order-preserving
 * key of the medium list's element above the code lengths of the patch's medium symbol and of its four fine symbols), both payloads are prefix-
 * summed in that order, and every K is a binary search and two prefix reads.  LIMIT: 12 bytes of LDS per 8x8 patch, at most
 * 12288 patches per image (n8 <= 12288: up to 768x1024 pixels; a 768x768 tile has 9216), codes of at most 4095 bits; beyond:
 * CGIC_ERR_UNSUPPORTED.  Every argument is checked before anything is enqueued.  Not inside a launch group.
 *
 * cgic_router_ranks (host only): the ranks cgic_router_f32 derives from a ratio pair for a segment of n16 coarse patches --
 * k_coarse = round(n16 c) in modes 0, 2, 3; k_medium = round(4 n16 c + n8 m) in mode 0, round(n8 m) in mode 1; 0 where the mode
 * uses none -- with Python's round-half-even on the float64 product.  CGIC_ERR_INVALID if k > n, as the router. */
size_t cgic_rate_curve_workspace_bytes(int64_t B, int64_t h16, int64_t w16);
int cgic_rate_curve(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f, const float *e16,
                    const float *e8, int64_t B, int64_t h16, int64_t w16, double coarse_ratio, int32_t *nbytes, void *workspace,
                    cgic_stream_t stream);
int cgic_router_ranks(double coarse_ratio, double medium_ratio, int64_t n16, int64_t *k_coarse, int64_t *k_medium);

/* Rate curves of tiled images (ABI 11): the curve of T tiles of MIXED shapes at M requested settings, folded per image -- rate
 * control for the tiling driver (section H; inference_high_resolution.py).  The reference applies ONE ratio pair to all tiles of an
 * image and routes every tile on its own thresholds (:236-251), so the bytes of the image at (c, m) are the sum over its tiles of
 * the tile's curve at K_tile = round(4 n16_tile c + n8_tile m): the medium rank depends on the tile's SHAPE only.
 *
 * cgic_rate_tile: one tile.  h16, w16: its shape in 16x16 patches; k_c: its coarse rank, round(n16 * coarse_ratio) (0 at coarse
 *   ratio 0), the expression cgic_rate_curve uses -- checked; shape: its shape class, 0 .. S - 1 (all tiles of a class have ONE
 *   shape); image: the image it belongs to, 0 .. N - 1; reserved: 0; off_*: where its ind_c / ind_m / ind_f / e16 / e8 start
 *   inside the concatenated buffers, in elements (each part dense: [h16,w16], [2h16,2w16], [4h16,4w16], [h16,w16], [2h16,2w16]).
 *
 * cgic_rate_curve_tiles:
 *   t, ind_c / ind_m / ind_f, e16, e8   device: the code table and the concatenated buffers of all tiles (types as cgic_rate_curve)
 *   count    host int64 [5]: the elements of ind_c, ind_m, ind_f, e16, e8 -- every tile's parts must lie inside
 *   tiles    host [T]: the descriptors, CHECKED here;  tiles_dev  device [T]: the same bytes, READ by the kernels (the caller's
 *            upload: it may be made once and reused while the geometry stays).  0 <= T <= 65535, 1 <= N <= 65535
 *   coarse_ratio   as cgic_rate_curve (the stream set: mode 0, or mode 1 at 0)
 *   ranks_dev   device int32 [S, M]: ranks[s, j] = the medium rank a tile of shape class s takes at setting j, 0 .. n8 of the
 *            class (host arithmetic: cgic_router_ranks).  1 <= S <= 16, 1 <= M <= 65536
 *   image_nbytes  device int64 [N, M, 5]: the five stream sizes of image n at setting j, summed over its tiles; all five -1 when a
 *            tile of the image has a negative entry there.  An image without tiles: zeros
 *   tile_nbytes   device int32 [T, M, 5] or NULL (then part of the workspace): tile_nbytes[t, j, :] == nbytes[b, ranks[s, j], :]
 *            of cgic_rate_curve for that tile; <= -10: a selected symbol outside the table (as there), or a rank outside 0 .. n8
 *   workspace device, cgic_rate_curve_tiles_workspace_bytes(T, M, tile_nbytes != NULL) bytes, 16-byte aligned; on return it starts
 *            with int32 [T, 4] per tile, as cgic_rate_curve's per image
 * Two launches: one workgroup per tile (steps 1-3 of cgic_rate_curve -- ONE device body for both entry points --, dynamic LDS
 * sized to the largest tile, the descriptor read with scalar loads; then the M ranks of the tile's class: a binary search and two
 * prefix reads each), and the fold (one thread per image and setting, int64 sums in descriptor order).  No workgroup waits on
 * another, no atomics on global memory: the results do not depend on T, on the order of the descriptors or on which tiles share a
 * call.  LIMITS per tile as cgic_rate_curve (n8 <= 12288, codes of at most 4095 bits).  Every argument
 * and every descriptor is checked before anything is enqueued: CGIC_ERR_INVALID / _UNSUPPORTED with nothing written.  Not inside
 * a launch group. */
typedef struct cgic_rate_tile {
    int32_t h16, w16;
    int32_t k_c;
    int32_t shape;
    int32_t image;
    int32_t reserved;
    int64_t off_c, off_m, off_f, off_e16, off_e8;
} cgic_rate_tile;
size_t cgic_rate_curve_tiles_workspace_bytes(int64_t T, int64_t M, int tile_nbytes_given);
int cgic_rate_curve_tiles(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f, const float *e16,
                          const float *e8, const int64_t *count, const cgic_rate_tile *tiles, const cgic_rate_tile *tiles_dev,
                          int64_t T, int64_t N, double coarse_ratio, const int32_t *ranks_dev, int64_t S, int64_t M,
                          int64_t *image_nbytes, int32_t *tile_nbytes, void *workspace, cgic_stream_t stream);

/* Device-side rate pick (ABI 12): route a same-size batch at the medium rank whose batch size is the largest one within a byte
 * budget -- curve, decision, masks and merged indices in one launch chain, the budget read from DEVICE memory: no host
 * synchronisation, no device-to-host copy and no launch parameter that depends on device results, so the chain can be captured in
 * a graph and replayed with another budget.  A same-size batch shares ONE medium rank per ratio pair (cgic_router_ranks does not
 * depend on the image), so the batch pick is a sum over the images per rank and an argmax under the budget.
 *
 * cgic_route_to_budget:
 *   t, ind_c / ind_m / ind_f, e16, e8, B, h16, w16, coarse_ratio   as cgic_rate_curve, with B >= 1 and coarse_ratio in [0, 1):
 *            the curve's mode -- 0, or 1 at coarse ratio 0.  ind_m, ind_f 16-byte aligned, e8 8-byte aligned
 *   ranks_dev   device int32 [R], 1 <= R <= n8 + 1: the medium ranks to choose among, ASCENDING, each one a rank a medium ratio
 *            reaches at this coarse ratio in the curve's mode (host arithmetic: cgic_router_ranks).  The CALLER owns this: the
 *            library cannot check a device list without a synchronisation.  (A rank outside 0 .. n8 is not dereferenced; it
 *            makes the choice -1.)
 *   budget_dev  device int64 [1]: the byte budget of the whole batch, read by the pick launch
 *   mask_c / mask_m / mask_f   device int32 [B,1,h16,w16] / [B,1,2h16,2w16] / [B,1,4h16,4w16], mask_m and mask_f 16-byte aligned:
 *            the masks cgic_router_f32 writes with per_image = 1 and refine = NULL at a ratio pair whose ranks are
 *            (k_c, the chosen K): coarse = e16 < s16[k_c - 1], medium = not coarse and e8 < t, fine = the rest
 *   ind      device int64 [B,4h16,4w16], 16-byte aligned: cgic_gather_grain_indices of those masks
 *   choice_dev  device int64 [4]: { j, K = ranks[j], fits, S[j] } with S[j] = the sum over the images of the five stream sizes at
 *            ranks[j] -- among the j with S[j] <= budget the largest S, on a tie the smaller j; if none fits the smallest S, on a tie
 *            the smaller j, and fits = 0.  If ANY requested entry of any image is negative (a selected symbol outside the table:
 *            what makes cgic_rate_curve's table negative there): { -1, -1, 0, -1 }, and the masks and ind are all zeros
 *   workspace device, cgic_route_to_budget_workspace_bytes(B, h16, w16, R) bytes, 16-byte aligned
 * Three launches ordered by the stream alone: the curve (one workgroup per image, steps 1-3 of cgic_rate_curve -- the same
 * device body -- then per requested rank the image's bytes and the medium threshold), the pick (one workgroup; integer
 * sums, so the result does not depend on any order) and the apply (elementwise, 16-byte stores).  No workgroup waits on another.
 * LIMITS as cgic_rate_curve.  Every host argument is checked before anything is enqueued.  Not inside a launch group. */
size_t cgic_route_to_budget_workspace_bytes(int64_t B, int64_t h16, int64_t w16, int64_t R);
int cgic_route_to_budget(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f, const float *e16,
                         const float *e8, int64_t B, int64_t h16, int64_t w16, double coarse_ratio, const int32_t *ranks_dev, int64_t R,
                         const int64_t *budget_dev, int32_t *mask_c, int32_t *mask_m, int32_t *mask_f, int64_t *ind,
                         int64_t *choice_dev, void *workspace, cgic_stream_t stream);

/* The container on the device (ABI 15): the blob of control_gic_amd/container.py -- version 1, flags 0:
 *     "CGIC" | u16 version | u16 flags | u32 n_entries | n_entries x 44-byte entry header | payload
 * with an entry header u32 image_id, y, x, height, width | u8 mode | 3 zero bytes | 5 x i32 stream length (-1 = not written), all
 * little endian, and the payload the streams of entry 0 in stream order, entry 1 ... -- built from, and taken apart into, slot
 * buffers as cgic_compress_streams writes and cgic_decompress_streams reads them, with no host loop and no synchronisation.
 *
 *   groups   host [G], G <= 64: per group  data   device [B, 5, slot] uint8, 16-byte aligned
 *                                          nbytes device [B, 5] int32
 *                                          B >= 0, slot a positive multiple of 16 below 2^31, mode 0 .. 6
 *   entries  host [E], E <= 65535, in container order: the five header words of the entry, the group it lives in and its index
 *            inside that group (0 <= index < B of the group; entries of different groups interleave freely, an image may appear
 *            more than once)
 * Both tables are consumed by the call (they travel in kernel-argument blocks: 64 entries a launch); nothing host-side has to
 * outlive it, and a captured call replays with the tables it was recorded with.
 *
 * cgic_container_pack:
 *   blob     device, `capacity` bytes, 16-byte aligned.  cgic_container_bound(groups, G, E) = 12 + 44 E + 5 E (largest slot) always
 *            suffices
 *   total    device int64 [1]: the bytes written -- blob[0 .. total) == container.pack of the same entries --, or a negative value:
 *            the smallest nbytes word of the named streams if any is below -1 (what cgic_compress_streams leaves for a symbol
 *            outside the table: CGIC_ERR_INVALID - 10; a length beyond its slot counts as CGIC_ERR_CAPACITY - 10), else
 *            CGIC_ERR_CAPACITY - 10 if the blob does not fit `capacity`.  On a negative total the content of the blob is
 *            unspecified, but no byte at or beyond `capacity` is touched; bytes at or beyond `total` are never written
 *   workspace device, cgic_container_workspace_bytes(E) bytes, 16-byte aligned
 * ceil(E / 64) + 2 launches ordered by the stream alone, no workgroup waits on another, no atomics on global memory: the stage
 * launches (slot address and length word of every stream into the workspace, the entry headers into the blob), the scan (ONE
 * workgroup: 5 E clamped lengths -> int64 offsets, the 12-byte header, total) and the copy (one thread per 16-byte word of the
 * blob gathers every stream that overlaps it -- a word can hold many: the shortest non-empty file has 2 bytes, empty and absent
 * streams make offsets coincide --: aligned 16-byte loads from the slots, a byte funnel shift, aligned 16-byte stores inside the
 * payload and byte stores in its first and last word).
 *
 * cgic_container_unpack: the inverse
 *   host_blob  host: the file, `bytes` long.  Checked in full before anything is enqueued: magic, version, n_entries == E, every
 *            length >= -1, 12 + 44 E + the lengths == bytes, the mode byte of every entry == its group's mode, its streams the
 *            set that mode writes (cgic_mode_streams), length + 8 <= slot of its group (CGIC_ERR_CAPACITY)
 *   blob     device: the same bytes in ONE contiguous upload, 16-byte aligned, readable up to the next multiple of 16
 *   groups, entries as above (of an entry only group and index are read); data / nbytes are the OUTPUTS: nbytes of all five streams
 *            of every named image (-1 included); every stream copied to the start of its slot and zeros from its end to the end of
 *            the 16-byte word that holds byte length + 7 (the slack the decoders' word fetches rely on); the rest of a slot, and
 *            images no entry names, are left alone
 * The same chain: stage (lengths re-read from the DEVICE copy, nbytes written), scan, and a scatter of one thread per 16-byte slot
 * word (aligned loads from the blob, the funnel, an aligned store).
 * Every host argument of both calls is checked before anything is enqueued.  Not inside a launch group. */
typedef struct cgic_container_group {
    void *data;
    int32_t *nbytes;
    int64_t B, slot;
    int mode;
} cgic_container_group;
typedef struct cgic_container_entry {
    uint32_t image_id, y, x, height, width;
    int32_t group, index;
} cgic_container_entry;
size_t cgic_container_bound(const cgic_container_group *groups, int G, int64_t E);
size_t cgic_container_workspace_bytes(int64_t E);
int cgic_container_pack(const cgic_container_group *groups, int G, const cgic_container_entry *entries, int64_t E, uint8_t *blob,
                        int64_t capacity, int64_t *total, void *workspace, cgic_stream_t stream);
int cgic_container_unpack(const uint8_t *host_blob, const uint8_t *blob, int64_t bytes, const cgic_container_group *groups, int G,
                          const cgic_container_entry *entries, int64_t E, void *workspace, cgic_stream_t stream);

/* LitEma (ABI 22): the exponential moving average of a model's parameters -- CGIC/models/ema.py:25-76, called five times after every
 * optimiser step (CGIC/models/model.py:147-153) -- over ALL tensors of a module in one launch.  The reference runs
 * shadow.sub_(one_minus_decay * (shadow - param)) per tensor (three launches, two temporaries) and reads num_updates on the host.
 *
 * A plan is built once from the list of tensor pairs and holds, in device memory, the work list of the launches: a table of entries
 * (shadow, param, n, offset in a stash) and a table of chunks (entry, offset, length) -- a tensor is cut into chunks of a fixed
 * number of elements (the last one shorter; a smaller tensor is one chunk; an empty one none) --, and one float, omd.
 *
 *   entries  host [n]: shadow, param device fp32 [n_i], 4-byte aligned (NULL allowed where n_i == 0), n_i >= 0.  The pairs must not
 *            overlap one another (shadow == param of one pair is harmless)
 * cgic_ema_plan_create checks every entry, computes the tables on the host and uploads them in one allocation on the current device,
 * SYNCHRONOUSLY: not for use while a stream is capturing.  CGIC_ERR_INVALID: n < 0, entries NULL with n > 0, an n_i < 0, a NULL
 * address with n_i > 0, an address that is not 4-byte aligned, more chunks than an int32 index can hold.  CGIC_ERR_NOMEM: no host memory for
 * the tables; CGIC_ERR_HIP: the allocation or the upload failed.  cgic_ema_plan_destroy frees
 * it (NULL: a no-op); the caller makes sure no launch that uses it is still in flight.
 * cgic_ema_plan_info: out host int64 [8] = { entries, elements, chunks, elements of a full chunk, chunks whose shadow AND param are
 * 16-byte aligned (they move 16 bytes per lane and access in the update and in direction 0; the others 4), workgroups of a launch,
 * elements of the stash of cgic_ema_copy, chunks whose param is 16-byte aligned (the same for directions 1 and 2) }.
 *
 * cgic_ema_update: for every element  shadow = shadow - (omd * (shadow - param)), three separately rounded fp32 operations (no
 * fused multiply-add), with omd computed on the device by a one-thread launch in front of it:
 *   decay        device float [1]
 *   num_updates  device int32 [1] or NULL.  If given and >= 0 it is incremented ONCE (by that one thread; wrapping like an int32
 *                tensor) and decay' = cand < decay ? cand : decay with cand = (float)(1 + n) / (float)(10 + n) of the incremented n,
 *                the additions wrapping in int32, the division in fp32 -- Python's min(self.decay, ...) of ema.py:30 (a NaN decay
 *                stays NaN); otherwise decay' = decay.   omd = 1.0f - decay'
 * Exactly two launches ordered by the stream (one when the plan has no chunk: the counter still moves), no allocation, no copy, no
 * synchronisation, no atomics: it may be captured into a graph and replayed.  The plan's omd is written by every call: calls on ONE
 * plan must be ordered by their streams (two streams may not run the same plan at once).
 *
 * cgic_ema_copy, bit for bit, one launch:   direction 0   param = shadow            (LitEma.copy_to)
 *                                           direction 1   stash = param             (LitEma.store)
 *                                           direction 2   param = stash             (LitEma.restore)
 *   stash   device fp32 [info[6]], 16-byte aligned, for directions 1 and 2 (ignored for 0): ONE buffer for all tensors; tensor i lives
 *           at the offset the plan gave it (the element counts before it, each rounded up to a multiple of 4).  Directions 1 and 2
 *           never touch shadow.
 * Every host argument is checked before anything is enqueued.  None of the five is available inside a launch group. */
typedef struct cgic_ema_entry {
    float *shadow;
    float *param;
    int64_t n;
} cgic_ema_entry;
typedef struct cgic_ema_plan cgic_ema_plan;
int cgic_ema_plan_create(const cgic_ema_entry *entries, int n, cgic_ema_plan **out);
void cgic_ema_plan_destroy(cgic_ema_plan *plan);
int cgic_ema_plan_info(const cgic_ema_plan *plan, int64_t *out);
int cgic_ema_update(const cgic_ema_plan *plan, const float *decay, int32_t *num_updates, cgic_stream_t stream);
int cgic_ema_copy(const cgic_ema_plan *plan, int direction, float *stash, cgic_stream_t stream);

/* Multi-tensor Adam (ABI 23): gradient clipping by value (clip_grad_value_), the step of torch.optim.Adam and LitEma's update over ALL
 * tensors of a parameter group in one pass -- per element: read g, p, m, v, s, write p, m, v, s.  Built like the EMA plan above (the same
 * chunks, the same grid, tables in one allocation); everything is fp32.
 *
 *   entries  host [n]: param, exp_avg, exp_avg_sq device fp32 [n_i], 4-byte aligned (NULL allowed where n_i == 0), n_i >= 0; shadow
 *            device fp32 [n_i] with ema_group the index of its EMA group, or shadow NULL and ema_group -1.  Tensors must not overlap.
 *   groups   host [ngroups], 0 <= ngroups <= 16: decay device float [1], num_updates device int32 [1] or NULL -- the two buffers of
 *            one LitEma; each group's counter moves once per step by the rule of cgic_ema_update.
 *   steps    device fp32 [n]: the step count of every entry, the caller's (torch's state["step"]); read and written by the prologue.
 * cgic_adam_plan_create checks everything, computes the tables on the host and uploads them in one allocation on the current device,
 * SYNCHRONOUSLY: not for use while a stream is capturing.  CGIC_ERR_INVALID: n < 0, a NULL list with a count > 0, an n_i < 0, a NULL
 * address with n_i > 0, an address that is not 4-byte aligned, an ema_group outside -1 .. ngroups - 1, a shadow without a group or a
 * group without a shadow, more than 16 groups, a NULL decay, NULL steps with n > 0, more chunks than an int32 index can hold.
 * CGIC_ERR_NOMEM / CGIC_ERR_HIP as for the EMA plan.  cgic_adam_plan_destroy frees it (NULL: a no-op); the caller makes sure nothing
 * that uses it is still in flight.
 * cgic_adam_plan_info: out host int64 [12] = { entries, elements, chunks, elements of a full chunk, chunks whose param, exp_avg,
 * exp_avg_sq and shadow are all 16-byte aligned (with a 16-byte aligned gradient they move 16 bytes per lane and access, the others
 * 4), workgroups of the body, EMA groups, entries with a shadow, uploads of the gradient table so far, uploads that had to wait for a
 * staging slot, bytes of the device tables, steps so far }.
 *
 * cgic_adam_step(plan, grads, hyper, stream):
 *   grads   host [n] device fp32 [n_i] gradient of every entry, 4-byte aligned, or NULL: no gradient this step (for an entry of 0
 *           elements any other address says that it has one: its step count moves, nothing is read).  The addresses are
 *           compared with those of the previous call; when they differ the new table is uploaded in stream order from one of four
 *           pinned staging slots of the plan (the host waits only when all four are still in flight); when they are equal nothing
 *           extra is enqueued.  While `stream` is capturing a changed table is refused (CGIC_ERR_INVALID), nothing enqueued.
 *   hyper   lr, beta1, beta2, eps, weight_decay, clip_value as doubles (torch's Python floats), clip != 0: clamp the gradient to
 *           +-clip_value first, lr_dev: device float [1] that replaces lr when not NULL (read by the prologue: a captured step follows
 *           a schedule).  CGIC_ERR_INVALID outside torch's ranges (lr, eps, weight_decay >= 0, betas in [0, 1)) or clip_value < 0.
 * Two launches ordered by the stream, no read of device memory on the host:
 *   prologue (one workgroup)  for every entry with a gradient: step += 1 (fp32); bias_correction1 = 1 - beta1^step and
 *           bias_correction2 = 1 - beta2^step in float64, the power by square-and-multiply from the lowest bit of the step count (a
 *           function of the count alone); step_size = lr / bias_correction1 and sqrt(bias_correction2), rounded to fp32, kept per
 *           entry.  For every EMA group: the counter and one_minus_decay of cgic_ema_update.
 *   body    per element, each operation rounded once in fp32, no fused multiply-add, torch's single-tensor operand order:
 *             g = grad;  clip: g = min(max(g, -c), c), a NaN stays;  weight_decay != 0: g = g + wd * p
 *             w = (float)(1 - beta1):  |w| < 0.5 ?  m = m + w * (g - m)  :  m = g - (g - m) * (1 - w)
 *             v = v * beta2;  v = v + ((float)(1 - beta2) * g) * g
 *             p = p + (-step_size) * (m / (sqrt(v) / bc2_sqrt + eps))
 *             with a shadow:  s = s - (omd * (s - p))  on the new p
 *           The gradient is not written.  An entry without a gradient keeps its step count, m, v and p; with a shadow it gets the last
 *           line alone.  Division and square root are correctly rounded.
 * The plan's tables are written by every call: calls on ONE plan must be ordered by their streams.  Every host argument is checked
 * before anything is enqueued.  None of the four is available inside a launch group. */
typedef struct cgic_adam_entry {
    float *param;
    float *exp_avg;
    float *exp_avg_sq;
    float *shadow;
    int64_t n;
    int32_t ema_group;
    int32_t reserved;
} cgic_adam_entry;
typedef struct cgic_adam_ema_group {
    const float *decay;
    int32_t *num_updates;
} cgic_adam_ema_group;
typedef struct cgic_adam_hyper {
    double lr, beta1, beta2, eps, weight_decay, clip_value;
    int32_t clip;
    int32_t reserved;
    const float *lr_dev;
} cgic_adam_hyper;
typedef struct cgic_adam_plan cgic_adam_plan;
int cgic_adam_plan_create(const cgic_adam_entry *entries, int n, const cgic_adam_ema_group *groups, int ngroups, float *steps, cgic_adam_plan **out);
void cgic_adam_plan_destroy(cgic_adam_plan *plan);
int cgic_adam_plan_info(const cgic_adam_plan *plan, int64_t *out);
int cgic_adam_step(cgic_adam_plan *plan, const float *const *grads, const cgic_adam_hyper *hyper, cgic_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CGIC_HIP_H */
