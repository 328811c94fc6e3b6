/*
 * bds.h -- C ABI of libbds.so: the MI355X (gfx950) hot path of bilateral-driving.
 *
 * The reference (BigCiLeng/bilateral-driving) is pure Python; its hot path is reached through
 * two Python import surfaces, not an FFI.  The functions declared here are the device entry
 * points those surfaces bind to (through ctypes, see bilateral_driving_amd/_lib.py and
 * INTEGRATION.md).  Each declaration cites the reference interface it serves
 * (paths relative to /root/reference/project).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major memory (fp32 unless noted),
 *     owned by the caller (the torch caching allocator); nothing is allocated inside;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), except the
 *     synchronous form of bds_isect_prepare, which hands the intersection count back to the host;
 *   - return value: BDS_OK or a negative BDS_E* code; never throws, never exits;
 *   - C = cameras, N = Gaussians, M = tile intersections, H/W = image size, tile = 16.
 */
#ifndef BDS_H
#define BDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDS_ABI_VERSION 7  /* 3: the projection's entries folded into four (bds_project_fwd, bds_project_view_fwd and
                               bds_project_view_bwd_list changed signatures)
                               4: the view path's host-count / device-count / split-storage twins folded into one entry each
                               (bds_splat_pack, bds_splat_pack_sh, bds_rasterize_fwd / _bwd, bds_sh_view_bwd_list, bds_view_grads_clear_list)
                               5: the tile stage's five entries folded into two (bds_isect_prepare and bds_isect_build changed signatures)
                               6: the colour transform's forward / backward, Adam's single-tensor step and the NaN / Inf check are one
                               entry each (bds_bilagrid_ms_fwd, bds_bilagrid_ms_bwd, bds_adam_step, bds_nonfinite_flags changed
                               signatures; bds_bilagrid_ms_ed_fwd, _ms_ed_train_fwd, _ms_ed_bwd, _ms_ed_bwd_deferred,
                               bds_adam_step_consume, bds_adam_step_rows, bds_nonfinite_flags_kinds and the unused
                               bds_bilagrid_tv_fwd / _bwd are gone; bds_bilagrid_ms_ed_bwd_deferrable is bds_bilagrid_ms_bwd_deferrable)
                               7: bds_pixel_loss_fwd / _bwd and bds_reg_loss_fwd / _bwd are gone: bds_image_loss_fwd / _bwd compute their
                               terms as two of its option sets */

#define BDS_OK 0
#define BDS_EINVAL (-1)      /* null / misaligned pointer, bad shape or unsupported parameter */
#define BDS_EWORKSPACE (-2)  /* workspace too small */
#define BDS_ELAUNCH (-3)     /* hipGetLastError() != hipSuccess after a launch / memcpy */
#define BDS_ECAPACITY (-4)   /* bds_isect_tiles: more intersections than the caller's buffers hold (see there) */

typedef void *bds_stream_t;

int bds_abi_version(void);
const char *bds_strerror(int code);

/* Test hooks that force the large-input fallback paths of the tile stage on small inputs (there is ONE kernel per
 * operation; these select which size regime a call is treated as).  which:
 * 0 = device-count tile stage: 1 [default] = launches behind the compaction sized by the visible-entry CAPACITY, 0 = by C*N;
 * 4 = depth ordering of the visible entries: 1 [default] = the two-launch radix passes used up to 8.4 M (camera, Gaussian)
 *     entries; 0 = the generic histogram / scan / scatter passes that larger inputs take;
 * 6 = tile lists: 1 [default] = packed 32-bit entries (tile << rank_bits | depth rank) whenever the visible count fits the
 *     rank bits; 0 = the (tile key, id) pair lists that larger visible counts take.
 * 3 = profiling only: ablation mask of the bilateral backward;
 * 7 = bilateral transform, bit mask [default 3]: bit 0 = the cell-aligned kernels (csrc/bilagrid_cells.hip) wherever a level
 *     qualifies (one grid per level); bit 1 = the pyramid forward as one pass over the image (csrc/bilagrid_tile.hip) when every
 *     factor is a power of two >= 2 dividing the image; bit 2 = do NOT defer the backward's last stage to the compositor
 *     (bds_bilagrid_ms_bwd_deferrable returns 0); 0 = the general kernels everywhere (what levels averaged over several
 *     grids always take).  Same results.
 * Other indices are unused. */
int bds_set_option(int which, int value);
int bds_get_option(int which);

/* Test hook (one wave, no reference counterpart): the two cross-lane transpose-reduces of csrc/bds_common.h on one input.
 * in [64][12]: lane l's 12 values; out16 [64] / out12 [64]: what butterfly_sum16 (the values padded with four zeros) and
 * butterfly_sum12 leave in each lane.  tests/test_gpu_48_reduce12.py compares them with its lane-by-lane model. */
int bds_reduce12_probe(const float *in, float *out16, float *out12, bds_stream_t stream);

/* Timing marks (measurement plumbing, no reference counterpart): HIP events that are recorded as event-record NODES when the
 * stream is being captured into a hipGraph, so that every replay re-records them and a kernel inside a captured view can be
 * bracketed (bench.py's roofline kernel).  bds_timer_elapsed_ms waits for `stop`; negative = not available. */
void *bds_timer_create(void);
int bds_timer_destroy(void *timer);
int bds_timer_mark(void *timer, bds_stream_t stream);
float bds_timer_elapsed_ms(void *start, void *stop);
int bds_last_hip_error(void);   /* HIP error code of the last failed runtime call of the timing-mark entry points (diagnostics) */

/* ---- spherical harmonics ----------------------------------------------------------------
 * gsplat.cuda._wrapper.spherical_harmonics(degrees_to_use, dirs, coeffs, masks=None)
 * imported at models/gaussians/basics.py:15, called at models/gaussians/vanilla.py:388
 * (and pvg.py:403, deformgs.py:142, nodes/rigid.py:462, deformable.py:83, smpl.py:364).
 * dirs [n,3] (normalised inside), coeffs [n,K,3], masks [n] uint8 or NULL, out [n,3].
 * Only the first (deg+1)^2 of the K bases are read.  v_dirs may be NULL. */
int bds_sh_fwd(int64_t n, int K, int deg, const float *dirs, const float *coeffs, const uint8_t *masks, float *out,
               bds_stream_t stream);
int bds_sh_bwd(int64_t n, int K, int deg, const float *dirs, const float *coeffs, const uint8_t *masks,
               const float *v_out, float *v_coeffs, float *v_dirs, bds_stream_t stream);

/* ---- projection -------------------------------------------------------------------------
 * first stage of gsplat.rendering.rasterization (called at models/trainers/base.py:393-408,
 * 811-826): quat+scale -> 3D covariance, world->camera, perspective Jacobian, eps2d blur,
 * conic, 3-sigma radius, near/far/screen culling.
 * means [N,3] quats [N,4] (wxyz, normalised inside) scales [N,3] viewmats [C,4,4] Ks [C,3,3]
 * -> radii [C,N] i32 (0 = culled), means2d [C,N,2], depths [C,N], conics [C,N,3],
 *    compensations [C,N] or NULL.  Culled entries are zero-filled.
 * compensations (rasterize_mode "antialiased", models/trainers/base.py:406): comp = sqrt(max(0, det S2 / det(S2 + eps2d I))), S2 the
 * FOV-clamped 2-D covariance before the blur, det S2 formed as a sum of squares (exact for needles, where the difference of the
 * entries' products is all rounding); the caller composites with opacity * comp.
 * opacities [N] and opac_eff [C,N] (both NULL or both set): the effective opacities of that mode in the same launch, opac_eff =
 * opacities * comp (what the tile stage and the compositor read then); compensations may be NULL with them. */
int bds_project_fwd(int C, int64_t N, const float *means, const float *quats, const float *scales, const float *opacities,
                    const float *viewmats, const float *Ks, int W, int H, float eps2d, float near_plane, float far_plane,
                    float radius_clip, int32_t *radii, float *means2d, float *depths, float *conics, float *compensations,
                    float *opac_eff, bds_stream_t stream);
/* v_means [N,3] v_quats [N,4] v_scales [N,3] are written (summed over cameras);
 * v_viewmats [C,4,4] (NULL = not needed) is zeroed and accumulated inside
 * (learnable camera poses: models/trainers/base.py:328-329,399).
 * compensations is not read (comp is recomputed) and may be NULL; v_compensations [C,N] or NULL: "antialiased" mode, adds the
 * compensation's gradient -- gsplat's v_S += v_comp 0.5 / (comp + 1e-6) ((1 - r) conic - eps2d det(conic) I), r = comp^2 (zero where
 * the clamp is active, r <= 0), evaluated without that cancelling difference (gs_math.h project_one_vjp). */
int bds_project_bwd(int C, int64_t N, const float *means, const float *quats, const float *scales,
                    const float *viewmats, const float *Ks, int W, int H, float eps2d, const int32_t *radii,
                    const float *conics, const float *compensations, const float *v_means2d, const float *v_depths,
                    const float *v_conics, const float *v_compensations, float *v_means, float *v_quats,
                    float *v_scales, float *v_viewmats, bds_stream_t stream);

/* ---- tile intersection + (tile|depth) ordering -------------------------------------------
 * isect_tiles + radix sort + isect_offset_encode stages of gsplat.rendering.rasterization.
 * Two calls because somebody must size the [M] outputs:
 *   bds_isect_prepare : depth-orders the visible Gaussians, counts their tiles in that order (per-member
 *                       records and per-256-member totals stay in `ws`) and leaves the two counts, M and the
 *                       number of visible entries, where the caller asked for them (below).
 *   bds_isect_build   : emits (camera*tiles+tile, id) pairs in depth order, stable-sorts them
 *                       by tile, writes flatten_ids [M] i32 (= cam*N+gaussian), isect_offsets
 *                       [C,th,tw] i32 and, if not NULL, isect_ids [M] i64
 *                       (cam|tile id << 32 | fp32 depth bits), identical to sorting the 64-bit
 *                       keys directly.
 * `ws` (bds_isect_prepare_workspace_bytes) must stay alive and untouched between the two calls;
 * `ws2` (bds_isect_build_workspace_bytes) is scratch for build.  M must be < 2^31.
 *
 * THREE WAYS OF GETTING THE COUNTS, selected by M_capacity / n_visible_capacity (both negative, or both >= 0) and `event`:
 *   synchronous  (capacities < 0, event NULL): `counts` = int64[2] in any host memory, zeroed on entry; the call synchronises
 *                `stream` and returns with counts = {M, visible entries}.
 *   asynchronous (capacities < 0, an event): same work, but instead of synchronising the GPU itself writes {M, visible entries}
 *                into `counts` (int64[2], page-locked host memory; a buffer the device cannot address is filled by the copy
 *                engine) and `event` (a hipEvent_t) is recorded on the stream.  The caller may enqueue independent work, then
 *                waits for the event, reads the counts and calls bds_isect_build: the GPU keeps running that work while the
 *                host sizes the lists.
 *   device-count (capacities >= 0; event must be NULL, C*N > 0): nothing is read back; see "device-count forms" below for the
 *                effective counts and overflow.  `counts` = page-locked int64[3] {M, visible entries, overflow} written by the
 *                GPU, or NULL (a buffer the device cannot address: BDS_EINVAL).  bds_isect_build is then called with
 *                device_counts = 1 and the same capacities as M / n_visible (both > 0; isect_ids and visible_ids NULL).
 * Any other combination is BDS_EINVAL. */
size_t bds_isect_prepare_workspace_bytes(int C, int64_t N);
/* Byte offset, inside the prepare workspace, of the ascending id list of the visible entries (int32 [n_visible], compact mode):
 * a caller that keeps `ws` alive reads the list in place and passes visible_ids = NULL to bds_isect_build (no copy). */
size_t bds_isect_visible_ids_offset(int C, int64_t N);
/* Byte offset, inside the prepare workspace, of the visible counts per 256 Gaussians (uint32 [cdiv(N, 256)]) that
 * bds_project_view_fwd with prep_ws leaves for bds_isect_prepare(..., compact | 2, ...): valid between those two calls.
 * An inspection hook like bds_isect_counts_offset: nothing in the product calls it; tests/test_gpu_43 reads the counts through it to
 * show that whole scan tiles were empty. */
size_t bds_isect_block_counts_offset(int C, int64_t N);
size_t bds_isect_build_workspace_bytes(int C, int64_t N, int64_t M);
/* conics [C,N,3] + opacities [C,N] (both or neither): when given, (tile, Gaussian) pairs in which no
 * pixel centre can reach alpha >= 1/255 are dropped ("exact tile culling"): rendered images and
 * gradients are unchanged, M shrinks; when NULL the lists are gsplat's bounding-square lists.
 * tiles_per_gauss [C,N] i32 may be NULL (the per-Gaussian counts are then not written). */
/* n_visible: number of (camera, Gaussian) entries with radii > 0.  Handing it to bds_isect_build
 * (or -1 when unknown) lets the build use PACKED lists when every entry's depth rank fits next to the tile key in one
 * 32-bit word (rank < 2^(32 - bits(C*tiles))): the tile sort then moves 4 bytes per entry instead of 8.  Same outputs. */
int bds_isect_prepare(int C, int64_t N, const float *means2d, const int32_t *radii, const float *depths,
                      const float *conics, const float *opacities, int tile_size, int tile_w, int tile_h,
                      int32_t *tiles_per_gauss, void *ws, size_t ws_bytes, int64_t M_capacity, int64_t n_visible_capacity,
                      int64_t *counts, void *event, int compact, bds_stream_t stream);
int bds_isect_build(int C, int64_t N, int64_t M, int64_t n_visible, const float *means2d, const int32_t *radii,
                    const float *depths,
                    const float *conics, const float *opacities, int tile_size, int tile_w, int tile_h, const void *ws,
                    size_t ws_bytes, void *ws2,
                    size_t ws2_bytes, int64_t *isect_ids, int32_t *flatten_ids, int32_t *isect_offsets,
                    int32_t *visible_ids, int device_counts, int compact, bds_stream_t stream);
/* COMPACT lists (no reference counterpart).  compact bit 0 (the same value in prepare and build; isect_ids must be NULL): every
 * intersection's list value is the entry's POSITION in the ascending list of the visible entries instead of its id cam*N+g
 * (same list order).  visible_ids (may be NULL; needs n_visible >= 0) receives that ascending list (position -> id) in either
 * mode.  Compact lists address splat records packed through visible_ids (bds_splat_pack), the compositor's gradient records
 * come back in that order, and everything downstream walks the visible ~15 % of the scene in memory order.
 * compact bit 1 (prepare only): the workspace already holds the visible counts and cleared tables of bds_project_view_fwd's
 * prep_ws (one launch less). */
/* One-call form: bds_isect_prepare and then, without returning to the caller in between, bds_isect_build into
 * buffers sized for an EXPECTED count (flatten_ids / isect_ids hold flatten_capacity entries, ws2 is
 * bds_isect_build_workspace_bytes(C, N, flatten_capacity)).  M <= flatten_capacity: BDS_OK, *n_isects = M, lists
 * written (entries [M, capacity) untouched).  Otherwise BDS_ECAPACITY, *n_isects = M, nothing built: allocate for M
 * and call bds_isect_build (ws is intact).  Saves the host's allocation work between the two stages, during which
 * the GPU idles. */
int bds_isect_tiles(int C, int64_t N, const float *means2d, const int32_t *radii, const float *depths,
                    const float *conics, const float *opacities, int tile_size, int tile_w, int tile_h,
                    int32_t *tiles_per_gauss, void *ws, size_t ws_bytes, void *ws2, size_t ws2_bytes,
                    int64_t flatten_capacity, int64_t *isect_ids, int32_t *flatten_ids, int32_t *isect_offsets,
                    int64_t *n_isects, int64_t *n_visible, bds_stream_t stream);

/* ---- alpha compositing -------------------------------------------------------------------
 * rasterize_to_pixels stage of gsplat.rendering.rasterization; outputs consumed at
 * models/trainers/base.py:409-419 (render, alphas) and :280-297 (means2d.absgrad).
 *
 * The compositor reads SPLAT RECORDS: 12 floats (48 bytes, 16-byte aligned) per list-addressable entry,
 *     mean2d.x, mean2d.y, ea, eb | ec, opacity, colour0, colour1 | colour2, colour3, 0, radius (int32 bits)
 * with (ea, eb, ec) = -log2(e) * (a/2, b, c/2) of the conic (a, b, c): alpha = opacity * 2^(ea dx^2 + eb dx dy + ec dy^2).
 * bds_splat_pack builds them from the per-entry arrays means2d [n,2] conics [n,3] colors [n,CH] opacities [n]: record r is
 * entry ids[r], or entry r when ids == NULL.  The per-tile lists (`flatten`) hold RECORD indices: cam*N + g for records in
 * array order (gsplat's flatten_ids), or depth ranks of the visible entries for records packed through a sorted id list.
 * CH in {1,3,4}; backgrounds [C,CH] or NULL -> render [C,H,W,CH], alphas [C,H,W], last_ids [C,H,W] i32.
 *
 * COARSE LISTS (no reference counterpart): list_tile_size is the tile size the lists were BUILT for (bds_isect_* called with it:
 * isect_offsets [C, ceil(H/list_tile_size), ceil(W/list_tile_size)]) -- tile_size (16, gsplat's lists) or a multiple of it.  With a
 * multiple, the tile stage emits and sorts one pair per (list tile, Gaussian) instead of one per (16-px tile, Gaussian), and every
 * 16 x 16 compositing wave filters the candidates of its list tile as it stages them, by the two conditions that define a pair of
 * gsplat's 16-px lists: the tile lies in the Gaussian's bounding square (radius slot of the record) and one of its pixel centres
 * reaches alpha >= 1/255 (the tile stage's exact span test).  Records packed WITH radii therefore give exactly the render / alphas /
 * gradients of 16-px lists (the fused view's use); records packed without (radii == NULL: unbounded square) give gsplat's semantics
 * for tile_size = list_tile_size, where a splat is clipped to its bounding square at that tile granularity (the rasterization()
 * API's tile_size argument).  last_ids holds positions in the coarse list. */
#define BDS_SPLAT_RECORD_FLOATS 12
#define BDS_GRAD_RECORD_FLOATS 16
/* Glue of gsplat's rasterization() as ONE node for one camera (rendering._RasterizeView; models/trainers/base.py:393-408):
 * records of the visible entries straight from post-activation colours [N,3] + depths [N] (channel 3 = depth, "RGB+ED");
 * the expected-depth normalise out4 = (rgb, D / max(alpha, 1e-10)) and its backward, which also widens a 3-channel ("RGB") image
 * gradient to the compositor's four channels: v_render4 = (v_out.rgb, v_out.d / max(alpha, 1e-10) | 0), v_alphas = v_alphas_in
 * (may be NULL) - [alpha >= 1e-10] D v_out.d / max(alpha, 1e-10)^2.  v_out: [P, channels], may be NULL (zeros). */
int bds_splat_pack_rgbd(int64_t n, const int32_t *ids, const float *means2d, const float *conics, const float *colors3,
                        const float *depths, const float *opacities, const int32_t *radii, float *records, bds_stream_t stream);
int bds_expected_depth_fwd(int64_t P, const float *render4, const float *alphas, float *out4, bds_stream_t stream);
int bds_expected_depth_bwd(int64_t P, int channels, int expected_depth, const float *render4, const float *alphas, const float *v_out,
                           const float *v_alphas_in, float *v_render4, float *v_alphas, bds_stream_t stream);
/* The same with the image as TWO arrays, rgb3 [P,3] and depth1 [P,1] (expected_depth = 0: the composited depth as it is): the
 * reference's trainer splits the render at once (models/trainers/base.py:409-419: torch.split(renders, [3, 1], dim=-1)); handed out as
 * two outputs of the rasterization node (rendering.SplitRender) that split costs no copy forward and no slice backward.
 * v_rgb3 / v_depth1 / v_alphas_in may be NULL (zero). */
int bds_expected_depth_split_fwd(int64_t P, int expected_depth, const float *render4, const float *alphas, float *rgb3, float *depth1,
                                 bds_stream_t stream);
int bds_expected_depth_split_bwd(int64_t P, int expected_depth, const float *render4, const float *alphas, const float *v_rgb3,
                                 const float *v_depth1, const float *v_alphas_in, float *v_render4, float *v_alphas, bds_stream_t stream);
/* n_dev (here and in every entry below that takes one; NULL: n is the count): the device-count form -- the count is read from n_dev
 * (visible effective, see "device-count forms"), n is then the capacity and sizes the launch.
 * Optionally clears, on the way, the gradient record of every packed row (zero_records [n, BDS_GRAD_RECORD_FLOATS]: what
 * bds_rasterize_bwd accumulates into) and a tail of zero_tail_floats (multiple of 4) floats (the camera-pose gradient slots): no fill
 * launches of their own.  schedule (optional): the schedule buffer the following bds_rasterize_fwd fills in its binned form -- its
 * header is cleared here too.  (The clearing arguments serve the device-count view; the kernel takes them with a host count as well.) */
int bds_splat_pack(int64_t n, const uint64_t *n_dev, int CH, const int32_t *ids, const float *means2d, const float *conics,
                   const float *colors, const float *opacities, const int32_t *radii /* [n entries] or NULL */, float *records,
                   float *zero_records, float *zero_tail, int64_t zero_tail_floats, int32_t *schedule, bds_stream_t stream);
/* Splat records of the fused view with the SH colour evaluated on the way (vanilla.py:383-389: SH of normalise(means - cam_pos), + 0.5,
 * clamp to [0,1]; channel 3 = depth): record r = visible Gaussian ids[r]; sh_rgb [n,3] receives the un-clamped colours in list order
 * (for bds_sh_view_bwd_list with sh_rgb_by_rank).  Replaces bds_sh_view_fwd + bds_splat_pack on that path: the colours of the ~85 %
 * culled Gaussians are never evaluated or stored.  n_dev and the clearing arguments as bds_splat_pack.
 *   coeffs_rest NULL: coeffs [N,K,3] with K*3 a multiple of 4 and 16-byte aligned rows.
 *   coeffs_rest non-NULL (K >= 2): the coefficients where the reference's Gaussian classes hold them (models/gaussians/vanilla.py:96-104:
 *       `_features_dc` [N,3] and `_features_rest` [N,K-1,3], two parameters with their own learning rates; :382 concatenates them on
 *       every call -- 192 bytes per Gaussian written and read back before anything is culled): band 0 from coeffs, bands 1.. from
 *       coeffs_rest, rows of 4-byte alignment, visible rows only. */
int bds_splat_pack_sh(int64_t n, const uint64_t *n_dev, const int32_t *ids, int K, int degrees_to_use, const float *means,
                      const float *cam_pos, const float *coeffs, const float *coeffs_rest, const float *means2d, const float *conics,
                      const float *depths, const float *opacities, const int32_t *radii, float *records, float *sh_rgb,
                      float *zero_records, float *zero_tail, int64_t zero_tail_floats, int32_t *schedule, bds_stream_t stream);
/* M_dev (forward and backward; NULL: M is the list length): the device-count form -- the length is read from M_dev (M effective, see
 * "device-count forms"), M is then the capacity (> 0).  tile_order, split_len, split_cap and split_pool belong to that form: without
 * M_dev the forward takes tile_order = NULL and split_len = 0 only (it never writes a schedule: bds_rasterize_bwd_schedule serves
 * those lists), the backward split_len = 0 only.
 * tile_order of the forward (optional: the schedule buffer of bds_rasterize_bwd_schedule): every compositing wave knows how far into its
 * list its tile blended when it ends, and leaves the backward's schedule itself: BINNED form (bds_set_option(8, 1), default) -- one
 * atomic drops the tile into the bin of its length (32 bins a factor 2^(1/4) apart, longest first) of its XCD's range of tiles, the
 * backward's workgroups find their tile by a prefix walk over the 32 counts, NO launch between the passes; the header must be clear when
 * the forward starts (the record pack's `schedule` argument).  bds_set_option(8, 0): the waves leave their keys and
 * bds_rasterize_bwd_schedule_sort -- one launch, a no-op in the binned form -- writes the sorted schedule.
 * split_len (> 0: one camera, four channels, lists of tiles larger than 16 px, the binned schedule, i.e. the fused view; 0 = off): a
 * tile whose list-tile list holds >= split_len entries is composited by FOUR waves, one 16 x 4 strip each (one pixel per lane; the
 * candidates filtered per strip), instead of one: a one-workgroup kernel lists those tiles behind the schedule words (at most
 * split_cap of them; a long tile beyond that is taken by one wave like any other) and the launch is [4 x split_cap strip workgroups,
 * first | one workgroup per tile].  For views in which a few tiles collect thousands of small splats (the vanishing point of a
 * street: the launch waits for those waves).  Same pixels in the same order: images bit-identical, gradients to the order of their
 * atomics.  Pass the SAME values and the same tile_order buffer to the backward.  No reference counterpart (gsplat runs 256 threads
 * per tile everywhere).
 * split_pool (> 0, with split_len; 0 = off): int32 words of a pool behind the schedule words -- the tile_order buffer then holds
 * bds_rasterize_schedule_ints(..) + bds_rasterize_split_pool_ints(.., split_cap, split_pool, M) words.  The long tiles of a list tile
 * share one walk of its list (per entry the mask of the sub-tiles it reaches), then one workgroup per long tile leaves the tile's own
 * candidates in the pool, in list order; the tile's strips (forward and backward) walk that instead of the whole list-tile list (the
 * front camera of a lidar-initialised street: 36 k entries per strip wave -> the ~8 k that reach the tile).  A tile the pool has no
 * room for keeps the list-tile list: never an error.  last_ids of a refined tile are positions in the pool. */
int bds_rasterize_fwd(int C, int64_t n_records, int64_t M, const uint64_t *M_dev, int CH, const float *records, const float *backgrounds,
                      int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h, const int32_t *isect_offsets,
                      const int32_t *flatten, float *render, float *alphas, float *t_final, int32_t *last_ids, int32_t *tile_order,
                      int split_len, int split_cap, int64_t split_pool, bds_stream_t stream);
/* (t_final [C,H,W], optional -- NULL: not written: every pixel's final transmittance ITSELF.  alphas = 1 - T rounds the low bits of a
 * small T away (T = 1e-4: 6e-4 relative), and the backward divides its way up from T: handed the same buffer, the backward starts
 * from the exact value -- element-wise gradient errors of dense scenes drop from ~1e-2 to the fp32 formulation's ~1e-3,
 * profiles/r09_gs_gradient_errors.json.  gsplat's backward starts from 1 - render_alphas.) */
/* Backward into GRADIENT RECORDS v_records [n_records, 16] (64-byte stride, zero-filled by the caller, accumulated with
 * atomics), in the units of the un-scaled inputs:
 *     0-3 d/d colour | 4-6 d/d conic (a, b, c) | 7-8 d/d mean2d | 9-10 sum over pixels of |d/d mean2d| (absgrad != 0) |
 *     11 d/d opacity | 12-15 unused.
 * tile_order may be NULL (tiles are taken in image order, one contiguous band per XCD), the schedule written by
 * bds_rasterize_bwd_schedule, or the buffer the device-count forward filled; M_dev and split_* as the forward's. */
int bds_rasterize_bwd(int C, int64_t n_records, int64_t M, const uint64_t *M_dev, int CH, const float *records, const float *backgrounds,
                      int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h, const int32_t *isect_offsets,
                      const int32_t *flatten, const float *alphas, const float *t_final, const int32_t *last_ids, const float *v_render,
                      const float *v_alphas, float *v_records, int absgrad, const int32_t *tile_order, int split_len, int split_cap,
                      int64_t split_pool, bds_stream_t stream);
/* Launch schedule for bds_rasterize_bwd (no reference counterpart; results do not depend on it).  One wave owns a
 * tile and the chip holds only about two rounds of tiles, so the launch ends with a tail of long tiles that started
 * late.  After the forward pass each tile's visited length is known exactly (max last_id - list start); this call
 * orders every XCD's contiguous range of tiles longest-first.  tile_order: int32[bds_rasterize_schedule_ints(C, tile_w, tile_h)]:
 * word 0 tags the form (1 = sorted: the order follows, then scratch; 0 = binned, written by bds_rasterize_fwd with M_dev), which the
 * backward kernels read -- hand the buffer over as it is. */
int64_t bds_rasterize_schedule_ints(int C, int tile_w, int tile_h);
int bds_rasterize_bwd_schedule(int C, int W, int H, int tile_size, int list_tile_size, int tile_w, int tile_h, const int32_t *isect_offsets,
                               const int32_t *last_ids, int32_t *tile_order, bds_stream_t stream);

/* ---- bilateral grid ----------------------------------------------------------------------
 * Point slice: bilateral/lib_bilagrid.py:317-368 BilateralGrid.forward (F.grid_sample,
 * trilinear, align_corners=True, padding_mode="border") used by slice() :171-230.
 * grid [12,L,gy,gx]; xy [P,2] in [0,1]; rgb [P,3] (guidance = BT.601 gray) -> affine [P,12].
 * bwd accumulates into v_grid (caller zero-fills) and writes v_rgb [P,3] (guidance route only). */
int bds_bilagrid_slice_fwd(int64_t P, const float *grid, int gx, int gy, int gl, const float *xy, const float *rgb,
                           float *affine, bds_stream_t stream);
int bds_bilagrid_slice_bwd(int64_t P, const float *grid, int gx, int gy, int gl, const float *xy, const float *rgb,
                           const float *v_affine, float *v_grid, float *v_rgb, bds_stream_t stream);

/* The same slice for FEATURE grids of any channel count NC (bilateral/lib_bilagrid.py:370-461 NeuralBilateralGrid.forward,
 * used by slice_feature :232-253): grid [NC,L,gy,gx] -> out [P,NC]; v_grid accumulated, v_rgb written (guidance route). */
int bds_bilagrid_slice_feat_fwd(int64_t P, int NC, const float *grid, int gx, int gy, int gl, const float *xy,
                                const float *rgb, float *out, bds_stream_t stream);
int bds_bilagrid_slice_feat_bwd(int64_t P, int NC, const float *grid, int gx, int gy, int gl, const float *xy,
                                const float *rgb, const float *v_out, float *v_grid, float *v_rgb, bds_stream_t stream);

/* The same slice over a whole IMAGE: xy is implied -- pixel (x, y) samples at (linspace(0,1,W)[x], linspace(0,1,H)[y]), which is what
 * the neural modules slice at (models/modules.py:643-650, 728-760: torch.meshgrid of two linspaces) -- so a workgroup can stage the
 * two grid rows a pixel row touches in LDS (the band [NC][gl][2][gx]) and scatter the gradient there.  rgb [H,W,3] -> out [H,W,NC]
 * (16-byte aligned when NC % 4 == 0).  bwd ACCUMULATES into v_grid [NC,gl,gy,gx] (caller zeroes; may be NULL) and writes v_rgb [H,W,3]
 * (the guidance route; may be NULL).  bds_bilagrid_slice_feat_image_ok(NC, gx, gy, gl) != 0 when the band fits (NC*gl*2*gx <= 6144
 * floats: the shipped 16x16x8 grid with 24 features exactly); otherwise the calls return BDS_EINVAL and the point form applies. */
int bds_bilagrid_slice_feat_image_ok(int NC, int gx, int gy, int gl);
int bds_bilagrid_slice_feat_image_fwd(int H, int W, int NC, const float *grid, int gx, int gy, int gl, const float *rgb, float *out,
                                      bds_stream_t stream);
int bds_bilagrid_slice_feat_image_bwd(int H, int W, int NC, const float *grid, int gx, int gy, int gl, const float *rgb,
                                      const float *v_out, float *v_grid, float *v_rgb, bds_stream_t stream);

/* Fused image transform: models/modules.py:505-522 MultiScaleBilateralAffineTransform.forward
 * (train branch: get_sample_grid :494-504, slice, fill_matrix_res :409-420), the single-scale
 * BilateralAffineTransform.forward :317-335 (factor 1), the sequential application at
 * models/trainers/scene_graph.py:95-98,112-117, and optionally the clamp + sky blend in front of
 * it (trainers/base.py:417, scene_graph.py:292-294).
 *
 * Level l: grid [n_avg, 12, L, gy, gx] (n_avg = 1 for training; > 1 averages the low-res
 * slices of neighbouring frames' grids = the test branch, modules.py:523-535).
 * If sky != NULL the input colour is clamp(rgb, max=1) + sky * (1 - alpha). */
#define BDS_MAX_LEVELS 8
typedef struct {
  const float *grid; /* [n_avg,12,gl,gy,gx] */
  float *v_grid;     /* same shape, accumulated (caller zero-fills); may be NULL in fwd */
  int32_t gx, gy, gl, factor, n_avg;
} bds_bilagrid_level_t;

size_t bds_bilagrid_ms_workspace_bytes(int nlevels, const bds_bilagrid_level_t *levels, int H, int W);
/* Forward.  ws keeps the low-resolution affine maps (fwd -> bwd).  The forms, by `channels` (any other value, or a mix: BDS_EINVAL):
 *   3: `in` is the colour [H,W,3].  affine_out (NULL or nlevels x [H,W,12] pointers) receives the full-resolution per-level maps the
 *      reference module returns.  depth_out and target must be NULL.
 *   4: the RGB+ED form.  `in` is the compositor's 4-channel render [H*W,4] (RGB + accumulated depth, gsplat render_mode "RGB+ED");
 *      alpha and depth_out are required: depth_out [H*W] = in[.,3] / max(alpha, 1e-10) (the normalise inside gsplat's
 *      rasterization(); split as in models/trainers/base.py:414-419).  affine_out must be NULL.
 *   4 with target != NULL: the training loss of the direct step rides on the same launch (no further pass over the image).  The
 *      full-resolution kernel also compares the pixel it just produced with target [H*W,3] -- loss_out (required; loss_slots a power
 *      of two, slotted as in bds_l1_tv_train) += mean|rgb_out - target|, v_rgb_out [H*W,3] (required) = sign(rgb_out - target) *
 *      v_loss / (3 H W) -- and tv_nlevels (may be 0) extra levels' worth of workgroups add sum_l tv_weights[l] *
 *      TV(tv_levels[l].grid) to loss_out and v_loss * its gradient to tv_levels[l].v_grid (atomics; may be NULL).  target, v_rgb_out
 *      and rgb_out 16-byte aligned.  Same result as the form without a target followed by bds_l1_tv_train.
 *      (models/trainers/base.py:518-565 rgb term + `losses.affine`, models/modules.py:445,466-472.)
 *   With target == NULL the arguments from tv_nlevels to v_rgb_out are ignored. */
int bds_bilagrid_ms_fwd(int nlevels, const bds_bilagrid_level_t *levels, int H, int W, int channels, const float *in,
                        const float *alpha, const float *sky, void *ws, size_t ws_bytes, float *rgb_out, float *depth_out,
                        float *const *affine_out, const float *target, int tv_nlevels, const bds_bilagrid_level_t *tv_levels,
                        const float *tv_weights, float v_loss, float *loss_out, int loss_slots, float *v_rgb_out, bds_stream_t stream);
/* Backward, same workspace.  The forms, by `channels` (any other value, or a mix: BDS_EINVAL):
 *   3: v_in [H,W,3] written; v_alpha [H,W], v_sky [H,W,3] written when sky != NULL.  v_depth, v_opacity NULL and defer 0.
 *   4: the RGB+ED form.  Returns v_in [H*W,4] and, in v_alpha (required, as alpha), the TOTAL alpha gradient: colour transform (sky
 *      blend) + expected depth + the caller's own v_opacity; v_depth / v_opacity / v_sky may be NULL.
 *   4 with defer != 0: the backward WITHOUT its last stage, see bds_bilagrid_ms_bwd_deferrable below.  v_in [H*W,4] receives the
 *      direct-route gradient (channels 0-2); v_depth, v_opacity, v_alpha and v_sky must be NULL; BDS_EINVAL for a configuration that
 *      is not deferrable. */
int bds_bilagrid_ms_bwd(int nlevels, const bds_bilagrid_level_t *levels, int H, int W, int channels, const float *in,
                        const float *alpha, const float *sky, void *ws, size_t ws_bytes, const float *v_rgb_out, const float *v_depth,
                        const float *v_opacity, float *v_in, float *v_alpha, float *v_sky, int defer, bds_stream_t stream);

/* TV regulariser: bilateral/lib_bilagrid.py:152-168 total_variation_loss on grids [n, channels, gl, gy, gx] (12 channels there;
 * NeuralBilateralGrid.tv_loss has others).  tv_out [1] is accumulated (caller zero-fills) with weight*tv; v_grids +=
 * weight*v_tv*dtv/dgrid. */
int bds_grid_tv_fwd(int64_t n, int channels, int gx, int gy, int gl, const float *grids, float weight, float *tv_out,
                    bds_stream_t stream);
int bds_grid_tv_bwd(int64_t n, int channels, int gx, int gy, int gl, const float *grids, float weight, const float *v_tv,
                    float *v_grids, bds_stream_t stream);
/* The same for all levels of a multi-scale transform in ONE launch each way: levels[l].grid / v_grid [n_avg,12,gl,gy,gx]
 * (n_avg = number of images, factor unused), weights[l] as above; tv_out accumulates sum_l weights[l] * tv_l. */
int bds_bilagrid_tv_ms_fwd(int nlevels, const bds_bilagrid_level_t *levels, const float *weights, float *tv_out,
                           bds_stream_t stream);
int bds_bilagrid_tv_ms_bwd(int nlevels, const bds_bilagrid_level_t *levels, const float *weights, const float *v_tv,
                           bds_stream_t stream);

/* L1 + TV training loss of the direct step, value and gradient in ONE launch: the loss = mean|a - b| + sum_l weights[l] *
 * TV(levels[l].grid) is ADDED, workgroup by workgroup, to loss_out [loss_slots * BDS_LOSS_SLOT_STRIDE] (zeroed by the caller;
 * loss_slots a power of two; the value is the sum of the slots' first floats -- thousands of float atomics on ONE address serialise
 * at ~8 ns each); v_a [n] = sign(a - b) * v_loss / n; levels[l].v_grid (may be NULL) += v_loss * d(weights[l] * TV)/d(grid), with
 * atomics (concurrent views may add to the same slices).  nlevels may be 0.
 * (models/trainers/base.py:518-565 rgb term + the `losses.affine` TV term, models/modules.py:445,466-472.) */
#define BDS_LOSS_SLOT_STRIDE 64
int bds_l1_tv_train(int64_t n, const float *a, const float *b, int nlevels, const bds_bilagrid_level_t *levels, const float *weights,
                    float v_loss, float *loss_out, int loss_slots, float *v_a, bds_stream_t stream);

/* ---- one-view forms for the fused training step ------------------------------------------------------
 * The per-Gaussian glue of one reference iteration folded into the two streaming kernels that sit next to it
 * (C = 1; same arithmetic as the general forms above):
 *   project_view: scales = exp(log_scales), opacities = sigmoid(logits) (models/gaussians/vanilla.py:393-394) are
 *     computed by the projection (and returned: the compositor and the backward read them); the backward returns the
 *     gradients of the raw parameters and reads only the radius of a culled Gaussian.
 *   sh_view: view direction = means - cam_pos (vanilla.py:384, detached), visibility = radii > 0, output packed for
 *     the RGB+ED compositor as colors [N,4] = (clamp(sh + 0.5, 0, 1), depth) (vanilla.py:389); sh_rgb [N,3] keeps the
 *     un-clamped value for the backward. */
/* ROW FORM of the projection's outputs (optional, recognised by the addresses -- no argument says so): means2d, depths and conics may
 * be the COLUMNS of one 16-byte aligned [N,8] block of 32-byte rows {m2d.x, m2d.y, depth, radius (int bits) | conic a, b, c, opacity}:
 * pass means2d = block, depths = block + 2, conics = block + 4 (both or neither; separate arrays of more than one row can not have
 * these addresses).  bds_project_view_fwd then writes whole rows (radii [N] and opacities [N] are written as dense arrays as well),
 * and bds_isect_prepare / bds_isect_build / bds_splat_pack_sh given the same three pointers (and opacities = block + 7, or any
 * dense [N] array of other opacities) gather ONE line per visible Gaussian instead of one per array. */
/* Block bounds: rows kept in spatial order (Morton order of the centres: the host side's densify.spatial_order) make every 256-row
 * block a small box, and a camera then rejects most of the ~85 % of the Gaussians it does not see a BLOCK at a time.
 * bds_gaussian_block_bounds: block_bounds [cdiv(N, 256), 8] = {lo.xyz, largest activated scale | hi.xyz, -} of the centres of rows
 * [256 b, 256 (b + 1)); recompute whenever means / log_scales changed (once per frame). */
int bds_gaussian_block_bounds(int64_t N, const float *means, const float *log_scales, float *block_bounds, bds_stream_t stream);
/* Flags of the one-view projection entries (bds_project_view_fwd takes BDS_PROJ_ANTIALIASED only). */
#define BDS_PROJ_ACCUMULATE 1
#define BDS_PROJ_ACTIVATED 2
#define BDS_PROJ_ANTIALIASED 4
#define BDS_PROJ_SKIP_UNTOUCHED 8   /* bds_project_view_bwd_list_touched only (see there) */
/* The one-view forward (C = 1): scales [N] = exp(log_scales), opacities [N] = sigmoid(logits), and the projection's outputs.
 *   flags & BDS_PROJ_ANTIALIASED: rasterize_mode "antialiased" (models/trainers/base.py:406, :824) -- the opacity the tile stage and the
 *       compositor read is the EFFECTIVE one, sigmoid(logit) * comp: slot 7 of the [N,8] row form, else opac_eff [N] (required in the
 *       column form, ignored in the row form); `opacities` keeps sigmoid(logit), which the backward reads.  Without the flag opac_eff
 *       must be NULL (the row form's slot 7 then holds sigmoid(logit)).
 *   prep_ws (NULL: none) also does the first launch of the tile stage (device-count form; N > 0): the number of visible Gaussians per
 *       256-Gaussian workgroup is left in prep_ws (bds_isect_prepare_workspace_bytes(1, N)), the stage's sort tables and
 *       tiles_per_gauss [N] (may be NULL) are cleared.  Follow with the device-count form of bds_isect_prepare(..., compact | 2, ...) on the SAME workspace.
 *       BDS_ECAPACITY when N is beyond the short sort path (call again with prep_ws = NULL then).  tiles_per_gauss is not touched
 *       without prep_ws.
 *   block_bounds (NULL: none) of bds_gaussian_block_bounds over the SAME means / log_scales: a 256-row block no centre of which can come
 *       out visible (conservative: csrc/gs_math.h box_may_be_visible follows the tests of the projection itself) is not read -- its
 *       rows get a culled Gaussian's outputs (radius 0, zeros; scales / opacities zero too).  Results are identical to the form without. */
int bds_project_view_fwd(int flags, int64_t N, const float *means, const float *quats, const float *log_scales, const float *logits,
                         const float *viewmat, const float *K, int W, int H, float eps2d, float near_plane, float far_plane,
                         float radius_clip, float *scales, float *opacities, float *opac_eff, int32_t *radii, float *means2d,
                         float *depths, float *conics, int32_t *tiles_per_gauss, void *prep_ws, size_t prep_ws_bytes,
                         const float *block_bounds, bds_stream_t stream);
/* The same call over PERSISTENT output buffers ("kept blocks"; block_bounds required): block_state [cdiv(N, 256)] u32 is caller-owned
 * memory that belongs to ONE set of output buffers (scales .. conics, opac_eff, tiles_per_gauss, in one form: rows or columns, with or
 * without prep_ws) -- one word per 256-row block, 0 = unknown (a fresh zeroed allocation), 1 = the block's rows hold a rejected block's
 * outputs.  A rejected block whose word is 1 stores no row (the buffers already hold exactly those zeros); a rejected block whose word is
 * not 1 stores them and sets the word; a surviving block stores its rows and clears the word.  Every word is read and written by its own
 * block's workgroup only.  The per-call workspace side (visible counts, cleared tables) is written on every call.  The outputs after a
 * call are byte for byte those of bds_project_view_fwd.  The state says what the BUFFERS hold, not which camera or parameters wrote
 * them: zero it whenever the buffers are replaced, or anything but this call (and the tile stage, which writes tiles_per_gauss of
 * visible rows only) may have written them. */
int bds_project_view_fwd_kept(int flags, int64_t N, const float *means, const float *quats, const float *log_scales, const float *logits,
                              const float *viewmat, const float *K, int W, int H, float eps2d, float near_plane, float far_plane,
                              float radius_clip, float *scales, float *opacities, float *opac_eff, int32_t *radii, float *means2d,
                              float *depths, float *conics, int32_t *tiles_per_gauss, void *prep_ws, size_t prep_ws_bytes,
                              const float *block_bounds, uint32_t *block_state, bds_stream_t stream);
int bds_sh_view_fwd(int64_t N, int K, int degrees_to_use, const float *means, const float *cam_pos, const float *coeffs,
                    const int32_t *radii, const float *depths, float *sh_rgb, float *colors, bds_stream_t stream);
/* Backward of the one-view forms over the VISIBLE entries only, list-driven (no reference counterpart; the reference's dense
 * backward writes zeros for every culled Gaussian).  ids [n_list] = depth-ordered ids of the visible entries (bds_isect_build:
 * visible_ids); v_records [n_list,16] = the compositor's gradient records of the same ranks (bds_rasterize_bwd with rank lists).
 * accumulate = 0 STORES the rows ids[.] of the gradient arrays (all other rows are the caller's business: zero-filled, or kept zero
 * with bds_view_grads_clear_list), accumulate = 1 ADDS to them (several views summed into one buffer before one exchange).
 *   sh_view_bwd_list     : v_coeffs [N,K,3] rows (colour clamp of vanilla.py:389 applied through sh_rgb).
 *   project_view_bwd_list: v_means [N,3] v_quats [N,4] v_log_scales [N,3] v_logits [N] rows (see there).
 * row_map (may be NULL) [N] i32: the parameter-gradient row of Gaussian g is row_map[g] instead of g -- the rows then land in a
 * compact exchange buffer (multi-GPU: the slot of g in the union of the ranks' visible sets) instead of the dense arrays. */
#define BDS_POSE_GRAD_SLOTS 64
/* ROW FORM of the four small parameter gradients (optional, recognised by the addresses like the projection's row form): v_means,
 * v_quats, v_log_scales, v_logits may be the columns of one 16-byte aligned [N,16] block of 64-byte rows {v_mean 3, v_logit | v_quat 4 |
 * v_log_scale 3, - | - - - -}: pass v_means = block, v_logits = block + 3, v_quats = block + 4, v_log_scales = block + 8.
 * bds_project_view_bwd_list then updates, and bds_view_grads_clear_list clears, ONE line per visible Gaussian instead of four partly
 * used ones; bds_adam_step with a width reads such columns. */
/* sh_rgb: the un-clamped colours the forward left -- [N,3] indexed by Gaussian (bds_sh_view_fwd), or, with sh_rgb_by_rank != 0,
 * [n_list,3] in list order (bds_splat_pack_sh).
 * v_coeffs_rest (NULL: v_coeffs is [N,K,3]): the split storage of bds_splat_pack_sh -- v_coeffs [N,3], v_coeffs_rest [N,K-1,3]
 * (visible rows stored or added to; ignored for K = 1).  Dense arrays only: not together with row_map.
 * n_dev (NULL: n_list is the count): the device-count form, as bds_project_view_bwd_list's.
 * accumulate: 0 / BDS_SH_ACCUMULATE as above, optionally | BDS_SH_SKIP_UNTOUCHED -- see UNTOUCHED ROWS below. */
#define BDS_SH_ACCUMULATE 1
#define BDS_SH_SKIP_UNTOUCHED 2
/* UNTOUCHED ROWS.  A view lists every visible Gaussian, but its pixels saturate after some tens of blends: most listed Gaussians lie
 * behind everything, no pixel blends them, and their gradient record stays at the exact zeros the record pack wrote (~87 % of the
 * ranks of a 2 M-Gaussian 1080p view; with the rows in spatial order 3 of 4 workgroups of 256 ranks hold nothing else).  Every
 * gradient of such a rank is +-0.  The skipping forms leave its rows alone:
 *   bds_sh_view_bwd_list with BDS_SH_SKIP_UNTOUCHED: a row whose colour gradient (record floats 0-2, behind the clamp mask) is all +-0
 *       is neither read nor written;
 *   bds_project_view_bwd_list_touched with BDS_PROJ_SKIP_UNTOUCHED: a rank whose record floats 0-11 are all +-0 reads no parameter,
 *       runs no VJP, stores nothing (parameter gradients, grad2d / absgrad2d, v_colors) and adds nothing to the pose slots.  With or
 *       without the flag, `touched` [n_list] bytes (may be NULL) receives per rank 1 = "floats 0-11 not all +-0", else 0;
 *   bds_view_grads_clear_list_touched: clears only the listed ranks whose `touched` byte is non-zero (NULL: every listed rank).
 * Adding +-0 is a no-op: accumulating, a skipped row differs from the dense form at most in the SIGN OF A ZERO.  Storing, the skipped
 * row keeps what it held, so skipping is allowed only where the destination rows are known to be zero: fresh zero tensors, an arena
 * the caller keeps zero, buffers cleared row-wise with the mask -- the invariant of graph_view.FrameGraph: every gradient row is zero
 * behind the begin stage; a row is written only where its record was non-zero; the mask (a caller-owned persistent buffer: the records
 * themselves do not outlive the frame) says 1 exactly there; exactly those ranks are cleared by the next begin stage.  A colour
 * gradient is part of floats 0-11, so the SH rows written are a subset of the mask.
 * NON-FINITE PARAMETERS: the dense forms compute 0 x Inf = NaN for an untouched row, the skipping forms leave it zero (the reference
 * rejects such parameters upstream, models/gaussians/vanilla.py:407-412; bds_nonfinite_flags). */
int bds_sh_view_bwd_list(int64_t n_list, const uint64_t *n_dev, const int32_t *ids, int K, int degrees_to_use, const float *means,
                         const float *cam_pos, const float *sh_rgb, int sh_rgb_by_rank, const float *v_records, float *v_coeffs,
                         float *v_coeffs_rest, const int32_t *row_map, int accumulate, bds_stream_t stream);
/* NaN / Inf check of the tensors a Gaussian class hands to the rasterizer (models/gaussians/vanilla.py:407-412 raises ValueError per
 * tensor; two reductions and two host waits each there): ONE streaming launch over up to 8 tensors; bit t of *flags_dev (cleared
 * first) is set when tensors[t] (counts[t] floats) holds a non-finite value; flags_pinned (optional, page-locked) receives a copy
 * behind the launch, for the host to read after its next wait on the stream.
 * kinds ([n_tensors], NULL = all 0): with a KIND the bit says "the tensor's ACTIVATED value would hold a NaN / Inf", for raw
 * parameters whose activation runs inside a kernel (vanilla.py:393-395, checked at :407-412 on the activated tensors):
 * 0 plain (NaN, +-Inf) | 1 argument of exp (NaN, +Inf, x >= 88.72284: exp overflows; -Inf is fine) | 2 quaternion rows [n/4, 4],
 * at any 4-byte alignment: row i is the four floats at tensors[t] + 4 i whatever the base's 16-byte phase -- a contiguous row slice or
 * a view into a flat buffer is checked like a fresh allocation (NaN / Inf components, or a row whose squared norm is 0 in fp32: 0/0,
 * x/0) | 3 argument of sigmoid (NaN only).  Every tensor is 4-byte aligned, counts[t] of a kind-2 tensor a multiple of 4 (BDS_EINVAL). */
int bds_nonfinite_flags(int n_tensors, const float *const *tensors, const int64_t *counts, const int *kinds, uint32_t *flags_dev,
                        uint32_t *flags_pinned, bds_stream_t stream);
/* ---- the scene view: one camera over several Gaussian classes (csrc/scene_view.hip) -------------------------------------------
 * models/trainers/base.py:355-366 concatenates every class's get_gaussians per key; the rows of the classes then lie one behind the other
 * in ONE global row range [0, N), N = sum of seg_rows.  A segment is RAW (a class whose colours are the reference's two SH parameters,
 * `_features_dc` [n,3] and `_features_rest` [n,K-1,3], evaluated at seg_degrees[i] as models/gaussians/vanilla.py:382-389 does) or
 * DENSE (a class that hands over post-activation colours [n,3]).  n_seg in [1, 8]; seg_rows / seg_kinds / seg_K / seg_degrees and the
 * two pointer tables are HOST arrays of n_seg entries (seg_K, seg_degrees and the second pointer are read for raw segments only); a
 * segment may have zero rows.  The projection, the tile stage and the compositors work on global row ids and serve such a scene as
 * they are (per-segment launches of bds_project_view_fwd / bds_project_fwd into rows [start, start + n) of one set of [N] arrays in
 * the column form; bds_project_view_bwd_list with BDS_PROJ_ACTIVATED over all rows); these two entries are the list-driven ends that
 * depend on a row's class.  n_dev: the device-count form, as bds_splat_pack's: a rank at or beyond the count reads and writes nothing.
 *   bds_scene_pack   : the splat records of bds_splat_pack_sh (same layout, same clearing arguments) for the visible rows ids[0..n):
 *       a raw row's colour is clamp(SH(normalise(mean - cam_pos)) + 0.5, 0, 1) from ITS segment's parameters (seg_colors[i] = band 0,
 *       seg_rest[i] = bands 1..), the un-clamped value kept in sh_rgb [n,3] by rank; a dense row's colour is seg_colors[i][local row]
 *       as it is (its sh_rgb row is zero).  means [N,3] are global rows; means2d / conics / depths / opacities / radii the [N]
 *       column-form outputs of the projection.
 *   bds_scene_sh_bwd : for the raw rows of the list, the SH backward (colour gradient = floats 0-2 of the gradient record of the same
 *       rank, the clamp applied through sh_rgb) STORED into the whole row of seg_v_dc[i] [n,3] / seg_v_rest[i] [n,K-1,3] (rows of
 *       culled Gaussians are the caller's: zero-filled), and the activation chain behind bds_project_view_bwd_list's ACTIVATED form,
 *       in place on the global arrays: v_scales[g] *= scales[g] (d exp), v_opacities[g] *= o (1 - o) (d sigmoid; scales / opacities =
 *       what bds_project_view_fwd left).  Dense rows are not touched. */
#define BDS_SCENE_DENSE 0
#define BDS_SCENE_RAW 1
int bds_scene_pack(int64_t n, const uint64_t *n_dev, const int32_t *ids, int n_seg, const int64_t *seg_rows, const int *seg_kinds,
                   const int *seg_K, const int *seg_degrees, const float *const *seg_colors, const float *const *seg_rest,
                   const float *means, const float *cam_pos, const float *means2d, const float *conics, const float *depths,
                   const float *opacities, const int32_t *radii, float *records, float *sh_rgb, float *zero_records, float *zero_tail,
                   int64_t zero_tail_floats, int32_t *schedule, bds_stream_t stream);
int bds_scene_sh_bwd(int64_t n_list, const uint64_t *n_dev, const int32_t *ids, int n_seg, const int64_t *seg_rows,
                     const int *seg_kinds, const int *seg_K, const int *seg_degrees, float *const *seg_v_dc, float *const *seg_v_rest,
                     const float *means, const float *cam_pos, const float *sh_rgb, const float *v_records, const float *scales,
                     const float *opacities, float *v_scales, float *v_opacities, bds_stream_t stream);
/* The list-driven projection backward over the visible entries (C = 1; ids, v_records, `accumulate` and row_map as above): the rows of
 * v_means [N,3] v_quats [N,4] v_scales [N,3] v_opacities [N].
 *   flags & BDS_PROJ_ACCUMULATE: ADD to the rows (accumulate = 1 above) instead of storing them.
 *   flags & BDS_PROJ_ACTIVATED: the backward of gsplat's rasterization() (models/trainers/base.py:393-408: the trainer passes ACTIVATED
 *       scales / opacities and post-activation colours [N,3]): the gradients of the activated scales and opacities are returned as they
 *       are and the colour gradient (record channels 0-2) is scattered to v_colors [N,3] (may be NULL).  Excludes BDS_PROJ_ACCUMULATE
 *       and row_map: the caller zero-fills the dense arrays; rows of culled Gaussians stay zero.
 *       Without it, the raw form of bds_project_view_fwd: scales / opacities are the activated values that forward left, v_scales /
 *       v_opacities receive the log-scale / logit gradients, v_colors is not used.
 *   flags & BDS_PROJ_ANTIALIASED: rasterize_mode "antialiased" (models/trainers/base.py:406).  Record channel 11 is the gradient of the
 *       effective opacity o * comp; comp is recomputed in the VJP: v_comp = v_eff * o enters the projection's gradient, the opacity
 *       gets v_eff * comp (times o (1 - o) for logits).
 *   n_dev (NULL: n_list is the count): the device-count form -- the count is read from n_dev (visible effective), n_list is then the
 *       capacity.
 *   grad2d / absgrad2d [N,2] (may be NULL): the screen-space gradient and the sum over pixels of its absolute value scattered to the
 *       dense arrays models/trainers/base.py:280-297 reads (rows of culled Gaussians untouched).
 *   v_viewmat_slots [BDS_POSE_GRAD_SLOTS,4,4] (may be NULL): camera-pose gradient partials, ADDED to (the caller zero-fills them, e.g.
 *       as the tail of the gradient-record allocation; replicated accumulators: one address would serialise in L2); the sum over the
 *       slots is d(loss)/d(viewmat), models/trainers/base.py:328-329,399. */
int bds_project_view_bwd_list(int flags, int64_t n_list, const uint64_t *n_dev, const int32_t *ids, const float *means,
                              const float *quats, const float *scales, const float *opacities, const float *viewmat, const float *K,
                              int W, int H, float eps2d, const float *v_records, float *v_means, float *v_quats, float *v_scales,
                              float *v_opacities, float *v_colors, float *v_viewmat_slots, float *grad2d, float *absgrad2d,
                              const int32_t *row_map, bds_stream_t stream);
/* The same with the untouched-rows mask (UNTOUCHED ROWS above): flags may add BDS_PROJ_SKIP_UNTOUCHED; touched [n_list] u8, may be NULL. */
int bds_project_view_bwd_list_touched(int flags, int64_t n_list, const uint64_t *n_dev, const int32_t *ids, const float *means,
                                      const float *quats, const float *scales, const float *opacities, const float *viewmat,
                                      const float *K, int W, int H, float eps2d, const float *v_records, float *v_means, float *v_quats,
                                      float *v_scales, float *v_opacities, float *v_colors, float *v_viewmat_slots, float *grad2d,
                                      float *absgrad2d, const int32_t *row_map, uint8_t *touched, bds_stream_t stream);
/* Zero the rows ids[0..n_list) of the five per-Gaussian gradient arrays (v_sh is [N,K,3]); n_dev (NULL: n_list is the count): the
 * device-count form, as above.
 * grad2d / absgrad2d [N,2], optional: the same rows of a view's PERSISTENT screen-space gradient arrays are cleared as well -- the
 * list-driven projection backward stores the visible rows, so a buffer cleared by the previous visit's list needs no dense fill.
 * The five parameter-gradient pointers may ALL be NULL: only the screen-space arrays are cleared then -- a loop whose optimizer
 * clears the gradients as it consumes them (bds_adam_step with consume != 0).  (Both serve the device-count view; the kernel
 * takes them with a host count as well.) */
int bds_view_grads_clear_list(int64_t n_list, const uint64_t *n_dev, const int32_t *ids, int K, float *v_means, float *v_quats,
                              float *v_log_scales, float *v_logits, float *v_sh, float *grad2d, float *absgrad2d, bds_stream_t stream);
/* touched [n_list] u8 by rank (NULL: as above): only the ranks with a non-zero byte are cleared (UNTOUCHED ROWS above). */
int bds_view_grads_clear_list_touched(int64_t n_list, const uint64_t *n_dev, const int32_t *ids, int K, float *v_means, float *v_quats,
                                      float *v_log_scales, float *v_logits, float *v_sh, float *grad2d, float *absgrad2d,
                                      const uint8_t *touched, bds_stream_t stream);
/* v_*[ids[s]] += s_*[s]: compact rows (s_means [n_list,3] s_quats [n_list,4] s_log_scales [n_list,3] s_logits [n_list]
 * s_sh [n_list,K,3], e.g. a reduced exchange buffer) added to the dense arrays; entries with ids[s] < 0 are skipped. */
int bds_view_grads_add_list(int64_t n_list, const int32_t *ids, int K, const float *s_means, const float *s_quats,
                            const float *s_log_scales, const float *s_logits, const float *s_sh, float *v_means, float *v_quats,
                            float *v_log_scales, float *v_logits, float *v_sh, bds_stream_t stream);

/* The grids of ONE image picked by an image index that lives in DEVICE memory: a captured (hipGraph) view whose image changes from
 * replay to replay -- the reference draws a random image every step (tools/train.py:257) and indexes the grid parameters with it
 * (models/modules.py:507-512, `int(image_infos["img_idx"][0][0])`, a host read-back there).  levels[l]: grid / v_grid = the FULL
 * parameter [n_img,12,gl,gy,gx] and its gradient, n_avg = n_img.  select: sel[l] [12,gl,gy,gx] = grid_l[*img_idx_dev];
 * select_bwd: v_grid_l[*img_idx_dev] += v_sel[l], then v_sel[l] = 0.  An index outside [0, n_img) selects / adds nothing (the
 * staging grids keep their contents; select_bwd still clears v_sel) and sets *error_pinned = 1 (page-locked int32, sticky, may be
 * NULL): the host cannot see a device-side index otherwise. */
int bds_bilagrid_select(int nlevels, const bds_bilagrid_level_t *levels, const int32_t *img_idx_dev, float *const *sel,
                        int32_t *error_pinned, bds_stream_t stream);
int bds_bilagrid_select_bwd(int nlevels, const bds_bilagrid_level_t *levels, const int32_t *img_idx_dev, float *const *v_sel,
                            int32_t *error_pinned, bds_stream_t stream);

/* The colour transform's backward WITHOUT its last stage (bds_bilagrid_ms_bwd with defer != 0), and the compositor's backward that
 * finishes it (one camera, RGB+ED; the fused view, models/trainers/base.py:393-419 + scene_graph.py:86-120,292-294 as one
 * backward).  The last stage of bds_bilagrid_ms_bwd -- guidance route added to the direct route, clamp(max=1) / sky blend / expected-depth backward -- is a
 * per-pixel function of arrays that exist by then; bds_rasterize_bwd_ms evaluates it for its tile's pixels while it waits for the
 * tile's first records, so v_render [H,W,4] and v_alpha [H,W] are never written and read back and one pass over the image (45 us,
 * 172 MB at 1080p) disappears.  bds_bilagrid_ms_bwd_deferrable: 1 when every level has one grid (gl <= 8) and a factor that is 1 or a power of two
 * dividing H and W (and bit 2 of bds_set_option(7, ..) is clear), else 0 (bad arguments included) -- call with defer = 0 then.  Deferred, the
 * grids' gradients are complete on return and v_direct is the call's v_in.  bds_rasterize_bwd_ms:
 * bds_rasterize_bwd (M_dev NULL: M_capacity is the host-side count; no split launch) for C = 1, CH = 4, no backgrounds, with the image
 * gradient formed from (levels, ms_ws: the transform's workspace), render [H,W,4] (the compositor's forward output), sky,
 * v_depth / v_alpha_in (may be NULL) and v_direct; writes v_sky [H,W,3] (may be NULL). */
int bds_bilagrid_ms_bwd_deferrable(int nlevels, const bds_bilagrid_level_t *levels, int H, int W);
int bds_rasterize_bwd_ms(int64_t n_records, int64_t M_capacity, const uint64_t *M_dev, const float *records, int W, int H,
                         int tile_size, int list_tile_size, int tile_w, int tile_h, const int32_t *isect_offsets,
                         const int32_t *flatten, const float *alphas, const float *t_final, const int32_t *last_ids, float *v_records,
                         int absgrad, const int32_t *tile_order, int nlevels, const bds_bilagrid_level_t *levels, void *ms_ws, size_t ms_ws_bytes,
                         const float *render, const float *sky, const float *v_depth, const float *v_alpha_in, const float *v_direct,
                         float *v_sky, bds_stream_t stream);

/* Names (as rocprofv3 prints them, without "bds::" and the argument list; comma-separated, launch order) of the kernels the bilateral
 * transform of this configuration launches under the current options (bds_set_option(7, ..)): forward (train != 0: with the L1 / TV
 * loss on the launch) or backward.  Measurement plumbing for bench.py's counter look-up; no reference counterpart. */
int bds_bilagrid_kernel_names(int nlevels, const bds_bilagrid_level_t *levels, int H, int W, int backward, int train, char *buf,
                              int buf_len);

/* Name (as rocprofv3 prints it, without the "bds::" prefix and the argument list) of the compositor kernel that a launch with
 * these switches runs (backward: 0 = forward, 1 = backward, 2 = backward with the colour transform's deferred epilogue,
 * bds_rasterize_bwd_ms); measurement plumbing for bench.py's counter look-up. */
int bds_rasterize_kernel_name(int backward, int CH, int absgrad, int list_tile_size, char *buf, int buf_len);

/* ---- device-count forms: one view without a host read-back (capturable in a hipGraph) -----------------------------------------
 * gsplat's rasterization() reads the intersection count back to size its lists (one host wait per view at
 * models/trainers/base.py:393-408).  These forms take CAPACITIES from the host (what the previous visit of the camera needed, plus
 * head-room) and the actual counts from device memory: the first words of the prepare workspace hold, as uint64,
 * {M, visible entries, M effective, visible effective, overflow} (byte offsets: bds_isect_counts_offset(0..4)).  The effective
 * counts are what every later stage sizes itself by; both are ZERO when a count outgrew its capacity -- the view then renders
 * nothing instead of overrunning a buffer, and the host, which looks at the prepare call's `counts` (page-locked int64[3] = M, visible,
 * overflow; written by the GPU; may be NULL) whenever it likes, provisions more and repeats the view.  Launches are sized by the
 * capacities; surplus workgroups see no elements.  Packed lists only (n_visible_capacity <= 2^(32 - bits(C*tiles))), else
 * BDS_ECAPACITY.  Lists, offsets and images are bit-identical to the host-count forms.  The tile stage's two calls are the ones of
 * "tile intersection" above (bds_isect_prepare with capacities, bds_isect_build with device_counts = 1; ws2 =
 * bds_isect_build_workspace_bytes(C, N, M_capacity), flatten_ids [M_capacity]).
 * Behind the tile stage the view takes the same entries as the host-count form, handed a count pointer: n_dev = visible effective
 * (bds_splat_pack, bds_splat_pack_sh, bds_sh_view_bwd_list, bds_project_view_bwd_list, bds_view_grads_clear_list), M_dev = M effective
 * (bds_rasterize_fwd / _bwd / _bwd_ms); the two helpers of the forward-written schedule follow below. */
size_t bds_isect_counts_offset(int which);
/* Words of the refined-list pool behind the schedule words (bds_rasterize_fwd: split_pool), and the sort of the keys the forward's
 * waves left (bds_set_option(8, 0); a no-op in the binned form). */
int64_t bds_rasterize_split_pool_ints(int C, int tile_w, int tile_h, int split_cap, int64_t split_pool, int64_t M_capacity);
int bds_rasterize_bwd_schedule_sort(int C, int tile_w, int tile_h, int32_t *tile_order, bds_stream_t stream);

/* ---- multi-GPU exchange of the visible rows (no reference counterpart; dist.FrameExchange) ---------------------------------------
 * mask [N] uint8: the element-wise OR over the ranks of "this rank's view sees Gaussian g" (radii > 0).  In two launches:
 * row_map [N] i32 = slot of every Gaussian in the union (cumsum(mask) - 1, clamped to [0, capacity - 1]); ids [capacity] i32 =
 * Gaussian at slot s, -1 beyond the union; rows [0, count) of the five compact sub-arrays (b_means [capacity,3] b_quats [capacity,4]
 * b_log_scales [capacity,3] b_logits [capacity] b_sh [capacity,K,3]) zeroed; count -> *count_dev (may be NULL) and count_pinned
 * (page-locked int64, written by the GPU; may be NULL).  A union larger than the capacity is reported through the count (rows
 * beyond it collide in the last slot: the caller repeats the frame with larger buffers).  ws: bds_union_slots_workspace_bytes(N). */
size_t bds_union_slots_workspace_bytes(int64_t N);
int bds_union_slots(int64_t N, const uint8_t *mask, int64_t capacity, int K, int32_t *row_map, int32_t *ids, float *b_means,
                    float *b_quats, float *b_log_scales, float *b_logits, float *b_sh, void *ws, size_t ws_bytes,
                    uint64_t *count_dev, int64_t *count_pinned, bds_stream_t stream);

/* ---- photometric L1 (the step right after the path) ---------------------------------
 * models/trainers/base.py:518-529: mean |a - b| over n floats.  out [1] is ACCUMULATED (caller zero-fills, so that
 * the TV terms of bds_grid_tv_fwd can land in the same scalar); a, b 16-byte aligned.
 * bwd: v_a = sign(a - b) * v_out / n with v_out a device scalar. */
int bds_l1_mean_fwd(int64_t n, const float *a, const float *b, float *out, bds_stream_t stream);
int bds_l1_mean_bwd(int64_t n, const float *a, const float *b, const float *v_out, float *v_a, bds_stream_t stream);

/* SSIM term of the image loss (models/trainers/base.py:114,541: pytorch_msssim.SSIM(data_range=1, size_average=True,
 * channel=3), loss = 1 - ssim(gt, pred)): 11x11 Gaussian window (sigma 1.5), valid region, K = (0.01, 0.03).
 * target / pred [H,W,CH] (H, W >= 11).  fwd ACCUMULATES the mean SSIM into ssim_out [1] (caller zero-fills) and, when
 * ws != NULL (bds_ssim_workspace_bytes), stores the per-pixel derivatives the backward needs; bwd writes
 * v_pred = v_ssim * d(mean SSIM)/d pred with v_ssim a device scalar (pass -upstream for the 1 - ssim loss). */
size_t bds_ssim_workspace_bytes(int H, int W, int CH);
int bds_ssim_fwd(int H, int W, int CH, const float *target, const float *pred, float *ssim_out, void *ws, size_t ws_bytes,
                 bds_stream_t stream);
int bds_ssim_bwd(int H, int W, int CH, const float *target, const float *pred, const void *ws, size_t ws_bytes,
                 const float *v_ssim, float *v_pred, bds_stream_t stream);

/* ---- Adam step on one parameter tensor (first slice) --------------------------------------
 * torch.optim.Adam as the reference trainer configures it (models/trainers/base.py:201-222: per-group lr / eps /
 * weight_decay, betas (0.9, 0.999), amsgrad off), one streaming pass, in place on param / exp_avg / exp_avg_sq.
 * `step` is the 1-based step count AFTER the increment (torch's state["step"]); the hyper-parameters are doubles (Python
 * floats): 1 - beta and the bias corrections are formed in double and rounded to fp32 once, as torch does.
 * width == 0: a contiguous gradient of n_rows floats (grad_stride is ignored; 16-byte vectors when every array is aligned).
 * width >= 1: a parameter [n_rows, width] whose gradient is a column range of a wider row block, element (r, c) at
 * grad[r * grad_stride + c] with grad_stride >= width (the [N,16] row form of the four small per-Gaussian gradients, see
 * bds_project_view_bwd_list).
 * consume != 0: the gradient is cleared as it is read ("consume and clear"): a training loop whose backward ACCUMULATES into
 * persistent gradient buffers (dist.FlatGradients / graph_view.FrameGraph) then needs no clearing pass before the next step --
 * what optimizer.zero_grad() (tools/train.py:266) costs the reference as one more pass over every gradient. */
int bds_adam_step(int64_t n_rows, int width, int64_t grad_stride, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                  double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, int consume,
                  bds_stream_t stream);

/* The same update for up to four parameter tensors [N, widths[t]] whose gradients are the column ranges [col0[t], col0[t] + widths[t])
 * of ONE [N,16] row block (64-byte rows; the four small per-Gaussian gradients, see bds_project_view_bwd_list), in one launch that
 * reads -- and, consuming, clears -- every row once: stepping the four tensors one after the other reads every 64-byte row four times.
 * grad_block is the block's base and must be 64-byte aligned (BDS_EINVAL otherwise).  Columns outside the given ranges -- tensors
 * that another optimizer steps, a frozen tensor, the unused columns -- are neither read into an update nor written: consuming clears
 * the given column ranges only. */
int bds_adam_step_rowblock(int64_t N, float *grad_block, int n_parts, float *const *params, float *const *exp_avgs,
                           float *const *exp_avg_sqs, const int *col0, const int *widths, const double *lrs, const double *beta1s,
                           const double *beta2s, const double *eps, const double *weight_decays, const int64_t *steps, int consume,
                           bds_stream_t stream);
/* bds_adam_step for up to 12 tensors in ONE launch (the trainer's ~10 small groups, models/trainers/base.py:201-226:
 * one launch per tensor is mostly launch gap).  Arrays of n_tensors entries; widths[t] = 0: a contiguous gradient, else element
 * (r, c) of tensor t's gradient at grads[t][r * grad_strides[t] + c] with c < widths[t]; steps[t]: the tensor's own 1-based step.
 * The same arithmetic per element: bit-equal to the single-tensor passes. */
int bds_adam_step_multi(int n_tensors, float *const *params, float *const *grads, float *const *exp_avgs, float *const *exp_avg_sqs,
                        const int64_t *counts, const int *widths, const int64_t *grad_strides, const double *lrs, const double *beta1s,
                        const double *beta2s, const double *eps, const double *weight_decays, const int64_t *steps, int consume,
                        bds_stream_t stream);
/* Deferred ("row-lazy") Adam for a parameter [N, row_floats] (row_floats <= 256) that only the rows of a view's visible-id list read
 * -- the SH coefficients -- with the numbers of the dense pass, bit for bit: the reference steps one dense Adam after every
 * single-view iteration (tools/train.py:252-283, models/trainers/base.py:222-226,502-516) and a row whose gradient is zero still
 * moves, so the steps a row missed are REPLAYED (same fp32 operations, same order, per-step scalars from `table`) when the row is
 * next needed.  last_step [N] i32: the step each row is current for; table [table_steps][4] floats (16-byte aligned): per-step
 * (lr_s/(1-b1^s) for columns < split_col, the same for columns >= split_col with lr_b, sqrt(1-b2^s), -), slot s % table_steps
 * written by the with_step launch of step s.  One call = "bring the rows of the list (ids [n_capacity] i32, entries < 0 skipped;
 * NULL: rows 0 .. n_capacity-1; n_dev: optional device-side count) to step t":
 *   with_step = 0: t = *clock_dev if clock_dev else `step`; rows with last < t replay the zero-gradient steps last+1 .. t.  Enqueued
 *                  inside a view's forward (after the visible list, before the record pack) with clock_dev, so that a captured
 *                  graph follows the optimizer; or densely before anything else reads the tensor / every table_steps-1 steps.
 *   with_step = 1: t = `step` (1-based, after the increment); rows with last < t replay last+1 .. t-1 and take step t from grad
 *                  [N, row_floats] (cleared as read when consume); rows already at t are skipped (a row listed by two views of a
 *                  frame steps once); table[t % table_steps] is written and *clock_dev = t.
 * The caller guarantees t - last < table_steps for every row it lists.  No reference counterpart (torch.optim.Adam is dense). */
int bds_adam_rows_advance(int64_t n_capacity, const uint64_t *n_dev, const int32_t *ids, int64_t N, int row_floats, int split_col,
                          float *param, float *grad, int consume, float *exp_avg, float *exp_avg_sq, int32_t *last_step,
                          int32_t *clock_dev, int64_t step, int with_step, float *table, int table_steps, double lr_a, double lr_b,
                          double beta1, double beta2, double eps, double weight_decay, bds_stream_t stream);

/* Per-step densification statistics of one set of Gaussians in one launch (models/trainers/base.py:279-297 +
 * models/gaussians/vanilla.py:163-191): grad2d [N,2] is info["means2d"].absgrad (or .grad) BEFORE the trainer's
 * width/2, height/2, batch_size scaling; radii [N] i32.  first != 0 reproduces the reference's initialising call
 * (xys_grad_norm = norm for every Gaussian, vis_counts = 1 for every Gaussian, max_2Dsize from zero). */
int bds_densify_stats(int64_t N, const float *grad2d, const int32_t *radii, int width, int height, int batch_size,
                      int last_size, int first, float *xys_grad_norm, float *vis_counts, float *max_2Dsize,
                      bds_stream_t stream);

/* ---- Adaptive density control: split / duplicate / cull + Adam-state surgery (second slice) -----
 * VanillaGaussians.refinement_after (models/gaussians/vanilla.py:205-304) with split_gaussians (:336-363), dup_gaussians
 * (:365-376), cull_gaussians (:306-334) and dup_in_optim / remove_from_optim (models/gaussians/basics.py:162-206), done as
 * ONE plan over the Gaussians followed by one write of every array straight into its final (culled) layout
 *   [ kept originals | kept split children, sample-major | kept dup children ]      (the order the reference's cat + cull gives).
 *
 * bds_refine_plan: flags [N] u8 (bit 0 split, 1 dup, 2 keep original, 3 keep its split children, 4 keep its dup child),
 * ranks [N,4] u32 (16-byte aligned; exclusive ranks among: split parents, kept originals, kept split parents, kept dup
 * parents) and totals [5] i64 on the device = {n_split, n_dup, kept originals KO, kept split parents KS, kept dup KD};
 * the new size is KO + samps*KS + KD and the host needs n_split for the noise tensor ([samps*n_split, 3], the reference's
 * torch.randn at vanilla.py:343).  The host decides the step-dependent switches exactly as the reference does:
 *   do_densify      step < stop_split_at and step % reset_interval > max(num_train_images, refine_interval)   (:212-215)
 *   size_thresh     densify_size_thresh * scene_scale;   split_by_screen: step < stop_screen_size_at            (:224-230)
 *   do_cull         step % reset_interval > max(num_train_images, refine_interval)                               (:279)
 *   cull_by_scale   step > reset_alpha_interval, cull_scale_thresh = cull_scale_thresh * scene_scale             (:314-320)
 *   cull_by_screen  additionally step < stop_screen_size_at                                                      (:321-324)
 * xys_grad_norm / vis_counts may be NULL when do_densify == 0; max_2Dsize may be NULL (treated as zeros).
 * extra_cull [N] u8 (may be NULL): a caller-computed cull mask over the INPUT rows, OR-ed into the decision for the originals when
 * do_cull != 0 (children are unaffected).  It serves the node classes' box test (models/nodes/rigid.py:302-303), which the
 * reference evaluates after the children were appended: the host runs a first plan for split / dup / the common culls, then
 * bds_refine_out_of_bound on the NEW means and a second, cull-only plan with that mask -- two order-preserving compactions leave
 * the rows, and their order, of the reference's single `culls` mask.
 * temp: bds_refine_plan_temp_bytes(N) bytes of scratch.  N < 2^31. */
size_t bds_refine_plan_temp_bytes(int64_t N);
int bds_refine_plan(int64_t N, const float *xys_grad_norm, const float *vis_counts, const float *max_2Dsize,
                    const float *log_scales, const float *logits, const uint8_t *extra_cull, int do_densify, float grad_thresh,
                    float size_thresh, int split_by_screen, float split_screen_size, int do_cull, float cull_alpha_thresh,
                    int cull_by_scale, float cull_scale_thresh, int cull_by_screen, float cull_screen_size, uint8_t *flags,
                    uint32_t *ranks, int64_t *totals, void *temp, size_t temp_bytes, bds_stream_t stream);

/* RigidNodes.get_out_of_bound_mask (models/nodes/rigid.py:374-383; DeformableNodes inherits it): mask[g] = 1 when
 * |means[g, i]| > instances_size[point_ids[g], i] / 2 for any axis i (means in the object frame, instances_size [n_instances,3],
 * point_ids [N] i64 -- the reference's [N,1] column).  An id outside [0, n_instances) is reported out of bound. */
int bds_refine_out_of_bound(int64_t N, const float *means, const int64_t *point_ids, int64_t n_instances,
                            const float *instances_size, uint8_t *mask, bds_stream_t stream);

/* New means [N',3] and log-scales [N',3]: split children are mean + R(q/|q|) (exp(log_scale) * noise) (vanilla.py:343-348);
 * a split parent and its children get log(exp(log_scale) / 1.6) (:356-359); dup children copy the (possibly shrunk) parent. */
int bds_refine_geometry(int64_t N, int samps, const uint8_t *flags, const uint32_t *ranks, const int64_t *totals,
                        const float *samples, const float *means, const float *quats, const float *log_scales,
                        float *new_means, float *new_log_scales, bds_stream_t stream);

/* Any other per-Gaussian array src [N,width] -> dst [N',width]: children receive the parent's row (zero_children = 0:
 * features, opacities, quaternions) or zeros (zero_children = 1: exp_avg / exp_avg_sq, basics.py:191-201). */
int bds_refine_rows(int64_t N, int width, int samps, const uint8_t *flags, const uint32_t *ranks, const int64_t *totals,
                    const float *src, float *dst, int zero_children, bds_stream_t stream);

/* Opacity reset (vanilla.py:286-299): logit = logit(min(sigmoid(logit), reset_value)) in place; the opacity group's
 * exp_avg / exp_avg_sq (either may be NULL) are zeroed. */
int bds_opacity_reset(int64_t N, float *logits, float reset_value, float *exp_avg, float *exp_avg_sq, bds_stream_t stream);

/* ---- Density control of the periodic-vibration Gaussians (models/gaussians/pvg.py) ------------------------------------
 * PeriodicVibrationGaussians.after_train (:100-133), refinement_after (:148-265) with split_gaussians (:298-354), dup_gaussians
 * (:356-372), cull_gaussians (:267-284), and the velocity_reg term of compute_reg_loss (:430-435).  scene_origin [3] is read on
 * the device (gamma, :90-98); thresholds the reference forms from Python floats arrive multiplied in double and rounded once.
 *
 * bds_pvg_densify_stats: after_train.  filter_mask [N] u8 (the bool mask get_gaussians leaves behind) with M rows set; row r of
 * grad2d [M,2] and radii [M] (i32, or f32 when radii_float != 0) is the r-th set row.  The gradient is scaled by (sx, sy) -- 1 for
 * the gradients the trainer has already scaled (models/trainers/base.py:285-286), width / 2 and height / 2 for raw ones -- and
 * taus_grad [N] enters by its absolute value.  first != 0 is the initialising call (:114-120): xys_grad_norm and t_grad_accum are
 * set for every kept row (0 elsewhere), vis_counts = 1 for EVERY row, max_2Dsize from zero; later calls touch only kept rows with
 * radius > 0.  temp: bds_pvg_mask_temp_bytes(N) bytes (the kept rows' offsets per workgroup).  N < 2^31, M <= N. */
size_t bds_pvg_mask_temp_bytes(int64_t N);
int bds_pvg_densify_stats(int64_t N, int64_t M, const uint8_t *filter_mask, const float *grad2d, float sx, float sy, const void *radii,
                          int radii_float, const float *taus_grad, int last_size, int first, float *xys_grad_norm,
                          float *t_grad_accum, float *vis_counts, float *max_2Dsize, void *temp, size_t temp_bytes,
                          bds_stream_t stream);

/* bds_pvg_refine_plan: the densification decisions of :165-202 WITHOUT a cull, in bds_refine_plan's layout -- flags bit 0 split,
 * bit 1 dup, bit 2 set for every row, bit 3 = split, bit 4 = dup; ranks [N,4] and totals [5] as there (KO = N) -- so that
 * bds_refine_rows appends the children in the reference's order.  kinds [N] u8: bit 0 = the (shrunk) parent is not over the size
 * threshold (:339-342, evaluated after the in-place shrink of :323), bit 1 = its time scale is not over t_size_thresh (:347).
 *   high = xys_grad_norm / vis > grad_thresh | t_grad_accum / vis > t_grad_thresh
 *   split = (max exp(scale) > size_thresh gamma | exp(beta) > t_size_thresh & high_t | max_2Dsize > split_screen_size) & high
 *   dup   = (max exp(scale AFTER the shrink of every split row) <= size_thresh gamma | exp(beta) <= t_size_thresh & high_t) & high
 * size_thresh = densify_size_thresh * scene_scale; split_by_screen: step < stop_screen_size_at (:179).  The host decides
 * do_densification as :155-159 does (including num_points < densify_until_num_points).  temp: bds_refine_plan_temp_bytes(N). */
int bds_pvg_refine_plan(int64_t N, const float *xys_grad_norm, const float *t_grad_accum, const float *vis_counts,
                        const float *max_2Dsize, const float *log_scales, const float *betas, const float *means,
                        const float *scene_origin, float scene_scale, float grad_thresh, float t_grad_thresh, float size_thresh,
                        float t_size_thresh, int split_by_screen, float split_screen_size, uint8_t *flags, uint8_t *kinds,
                        uint32_t *ranks, int64_t *totals, void *temp, size_t temp_bytes, bds_stream_t stream);

/* The four arrays a split changes, for the N + samps n_split + n_dup rows of such a plan: means [N',3], log-scales [N',3],
 * taus [N'], betas [N'].  samples [samps n_split, 4]: columns 0-2 the randn of :305, column 3 a unit normal z with
 * samples_t = exp(beta) z (:330-332).  Child: mean + R(q/|q|)(exp(scale before the shrink) n) + velocity exp(-0.5 exp(beta) / T)
 * samples_t (:313, :337); tau + samples_t (:333); log-scale log(exp(s) / 1.6), through one more exp / log for a kinds bit 0 child
 * (:343-345); beta log(exp(beta) / 1.6), log(exp(beta)) for a kinds bit 1 child and for every child when no_time_split (:347-353).
 * Split parents get the shrunk log-scale and keep tau and beta; dup children copy the possibly shrunk parent.  samps >= 1. */
int bds_pvg_refine_geometry(int64_t N, int samps, int no_time_split, double T, const uint8_t *flags, const uint8_t *kinds,
                            const uint32_t *ranks, const int64_t *totals, const float *samples, const float *means,
                            const float *quats, const float *log_scales, const float *velocity, const float *taus, const float *betas,
                            float *new_means, float *new_log_scales, float *new_taus, float *new_betas, bds_stream_t stream);

/* cull_gaussians (:267-284) on the N NEW rows, of which the first n_old carry max_2Dsize (children enter with 0): mask[g] = 1 when
 * sigmoid(logit) < cull_alpha_thresh, or (cull_by_scale: step > reset_alpha_interval) max exp(scale) > cull_scale_thresh gamma(mean)
 * with cull_scale_thresh already times scene_scale, or (additionally cull_by_screen: step < stop_screen_size_at)
 * max_2Dsize > cull_screen_size.  The mask is the extra_cull of a cull-only bds_refine_plan (cull_alpha_thresh = 0). */
int bds_pvg_cull_mask(int64_t N, int64_t n_old, const float *logits, const float *log_scales, const float *means,
                      const float *max_2Dsize, const float *scene_origin, float scene_scale, float cull_alpha_thresh, int cull_by_scale,
                      float cull_scale_thresh, int cull_by_screen, float cull_screen_size, uint8_t *mask, bds_stream_t stream);

/* velocity_reg (:430-435): out = {sum, count} (double) of |_velocity exp(-0.5 exp(beta) / T)| over the rows kept by filter_mask
 * whose radius (radii [M], as above) is > 0, summed in a fixed order without float atomics; vis [N] u8 marks those rows.
 * _bwd: the gradient of sum * scale[0] (scale: one float on the device) towards _velocity [N,3] and _betas [N]; rows outside the
 * set get zeros, and so does a row whose velocity is zero (torch's norm backward).  temp: bds_pvg_mask_temp_bytes(N). */
int bds_pvg_velocity_reg_fwd(int64_t N, int64_t M, double T, const uint8_t *filter_mask, const void *radii, int radii_float,
                             const float *velocity, const float *betas, uint8_t *vis, double *out, void *temp, size_t temp_bytes,
                             bds_stream_t stream);
int bds_pvg_velocity_reg_bwd(int64_t N, double T, const uint8_t *vis, const float *scale, const float *velocity, const float *betas,
                             float *g_velocity, float *g_betas, bds_stream_t stream);

/* ---- The whole image loss of BasicTrainer.compute_losses in one pass each way ---------------------------------------------------------
 * models/trainers/base.py:518-585 and :638-652 at every option of models/losses.py:33-178 (csrc/image_loss_math.h).  rgb, pixels
 * [H*W,3]; opacity, depth, sky_masks, lidar, egocar, dyn_opacity [H*W], 4-byte aligned.  valid = 1 - egocar (NULL: 1).  weights [6] are
 * HOST floats; terms [6] (device) come out weighted:
 *   terms[0] rgb L1 (:533-540)                 w0 mean |pixels*valid - rgb*valid| over 3 H W
 *   terms[1] sky opacity (:536-550)            mask_kind 0 off (sky_masks NULL), 1 torch's binary_cross_entropy (losses.py:81-83), 2
 *            SafeBCE with safe_limit in (0,1) (losses.py:33-79: its own backward, a gradient where the forward clipped, none where the
 *            re-clipped x equals y); x = opacity*valid, y = (1 - sky_masks)*valid, mean over H W
 *   terms[2] lidar depth (:552-565)            on where lidar != NULL.  DepthLoss (losses.py:91-178): hit = (lidar > 0)*valid, over
 *            {0.01 < lidar*hit < max_depth, depth*hit > 1e-4}; depth_normalize: clamp(d / max_depth, 1e-6, 1); depth_inverse: 1 / d;
 *            depth_type 0 l1, 1 l2, 2 smooth_l1 (beta 1); depth_reduction 0 mean_on_hit (NaN over an empty set, as torch's empty
 *            mean), 1 mean_on_hw, 2 sum
 *   terms[3] opacity entropy (:568-573)        on where entropy != 0: mean of -p log p, p = clamp(opacity, 1e-6, 1 - 1e-6)
 *   terms[4] inverse-depth smoothness (:576-585)  on where smoothness != 0: kornia.losses.inverse_depth_smoothness_loss(1 / (depth + 1e-5),
 *            pixels); kornia is an external package absent here: restated from its published definition, PARITY UNPINNED
 *   terms[5] dynamic-region L1 (:638-652)      on where dyn_opacity != NULL: over {dyn_opacity > dyn_threshold, valid != 0}; 0 when empty
 * A term that is off is 0.  No atomics: the forward's workgroups write rows of sums into temp (bds_image_loss_temp_bytes bytes), a
 * one-workgroup finish adds them in a fixed order into sums [9] (kept for the backward: seven numerators, the depth and the dynamic
 * count) and forms the terms; bit-identical run to run.  The backward writes (not accumulates) each given output once: v_rgb [H*W,3] =
 * terms 0 + 5, v_opacity [H*W] = terms 1 + 3, v_depth [H*W] = terms 2 + 4, scaled by v_terms [6] (device); any of them may be NULL. */
size_t bds_image_loss_temp_bytes(int H, int W);
int bds_image_loss_fwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                       const float *sky_masks, const float *lidar, const float *egocar, const float *dyn_opacity, int mask_kind,
                       double safe_limit, int depth_type, int depth_normalize, int depth_inverse, float max_depth, int depth_reduction,
                       int entropy, int smoothness, float dyn_threshold, const float *weights, float *terms, float *sums, void *temp,
                       size_t temp_bytes, bds_stream_t stream);
int bds_image_loss_bwd(int H, int W, const float *rgb, const float *pixels, const float *opacity, const float *depth,
                       const float *sky_masks, const float *lidar, const float *egocar, const float *dyn_opacity, int mask_kind,
                       double safe_limit, int depth_type, int depth_normalize, int depth_inverse, float max_depth, int depth_reduction,
                       int entropy, int smoothness, float dyn_threshold, const float *weights, const float *sums, const float *v_terms,
                       float *v_rgb, float *v_opacity, float *v_depth, bds_stream_t stream);

/* ---- Cube-map sky (the ROCm replacement of nvdiffrast's cube texture) -----------------------------
 * EnvLight.forward (models/modules.py:176-211): out[i] = bilinear cube-map lookup of tex [6,res,res,channels] along
 * dirs[i] @ rot^T (rot: 9 floats on the device, row-major, NULL = identity; the reference's to_opengl, :189,196) --
 * dr.texture(tex[None], l, filter_mode='linear', boundary_mode='cube') (:202).  OpenGL face order / orientation; taps that
 * fall off a face come from the neighbouring face; a non-finite direction yields zeros.  PARITY UNPINNED (nvdiffrast is
 * absent and unpinned, README.md:83): see csrc/envlight.hip.
 * bwd ACCUMULATES into v_tex (caller zeroes it); directions carry no gradient (the reference's viewdirs are data).
 * width > 0 tells bwd that dirs is a row-major image [n / width, width, 3] (n % width == 0): 16x16 pixel tiles then pre-sum
 * their taps in LDS before touching v_tex (channels == 3 only); width = 0: one global atomic per tap and channel. */
int bds_cubemap_fwd(int64_t n, int res, int channels, const float *dirs, const float *rot, const float *tex, float *out,
                    bds_stream_t stream);
int bds_cubemap_bwd(int64_t n, int res, int channels, int width, const float *dirs, const float *rot, const float *v_out,
                    float *v_tex, bds_stream_t stream);

/* ---- Colour-correct post-process of the evaluation path ----------------------------------------
 * One iteration of lib_bilagrid.color_correct (bilateral/lib_bilagrid.py:56-120; called per frame at
 * models/video_utils_color_correction.py:201) as one streaming pass:
 *   cur = warp ? clip(expand(cur_in) @ warp, 0, 1) : cur_in          expand(r,g,b) = [rr, rg, rb, gg, gb, bb, r, g, b, 1] (:98-104)
 *   mask0 [P] u8: bit c = channel c of the ORIGINAL image is in [eps, 1-eps] -- written when warp == NULL (first pass), read otherwise
 *   cur_out [P,3] (may be NULL) receives cur
 *   acc [3,65] doubles (may be NULL; ACCUMULATED into, caller zeroes): per output channel c, over the pixels with mask0 bit c set and
 *   cur_c, ref_c in [eps, 1-eps] (:110): the 55 upper-triangle entries (row-major) of sum expand expand^T, then the 10 entries of
 *   sum expand * ref_c.  The caller solves the three 10x10 systems (float64) -> next warp [10,3] row-major float. */
int bds_color_correct_step(int64_t P, const float *cur_in, const float *ref, const float *warp, float eps, uint8_t *mask0,
                           float *cur_out, double *acc, bds_stream_t stream);

/* ---- Fused head of the neural bilateral variants ---------------------------------------------------
 * NeuralBilateralAffineTransform / MultiScaleNeuralBilateralAffineTransform (models/modules.py:595-820): per pixel the sliced
 * features [P,F] go through `affine_network` = Linear(F,hidden) tanh Linear(hidden,hidden) tanh Linear(hidden,12), all without bias
 * (:621-627, :700-706; weights in torch's [out, in] layout: w1 [hidden,F], w2 [hidden,hidden], w3 [12,hidden]), and the 12 outputs
 * are the row-major 3x4 map the trainer applies with a residual (models/trainers/scene_graph.py:99-106):
 *   affine [P,12] (may be NULL)  = the network's output (what the modules' forward returns, reshaped [1,H,W,3,4] by the caller)
 *   out    [P,3]  (may be NULL)  = A[:, :3] rgb + A[:, 3] (+ rgb when residual != 0)
 * One kernel each way on the FP32 matrix cores (exact f32 products and sums, csrc/mlp_head.hip); hidden must be 64 (the shipped
 * configs, configs/omnire_neuralbilateral.yaml:251-252, omnire_ms_neuralbilateral.yaml:249-250) and F one of 8, 16, 24, 32
 * (feature_dim x number of levels), anything else returns BDS_EINVAL.  feats / affine / v_feats / v_affine 16-byte aligned.
 * bwd takes the gradient of either output (v_out and / or v_affine, the other NULL) and writes v_feats [P,F] and v_rgb [P,3] (the
 * direct path through the application only: the path through the features belongs to the slice operator; needs v_out) -- each may be
 * NULL -- and the weight gradients v_w1 / v_w2 / v_w3 (each may be NULL; stored, or added to when accumulate_w != 0).  The hidden
 * activations are recomputed, nothing is kept from the forward.  temp: bds_mlp_head_bwd_temp_bytes(P, F) bytes (per-wave partial
 * weight gradients, summed in a fixed order: the result is deterministic). */
size_t bds_mlp_head_bwd_temp_bytes(int64_t P, int F);
int bds_mlp_head_fwd(int64_t P, int F, int hidden, const float *feats, const float *rgb, const float *w1, const float *w2,
                     const float *w3, int residual, float *out, float *affine, bds_stream_t stream);
int bds_mlp_head_bwd(int64_t P, int F, int hidden, const float *feats, const float *rgb, const float *w1, const float *w2,
                     const float *w3, int residual, const float *v_out, const float *v_affine, float *v_feats, float *v_rgb,
                     float *v_w1, float *v_w2, float *v_w3, int accumulate_w, void *temp, size_t temp_bytes, bds_stream_t stream);

/* The whole `transform` of the neural variants for one image, the feature slice folded in (the sliced features never reach
 * memory): NeuralBilateralAffineTransform.forward / MultiScaleNeuralBilateralAffineTransform.forward with guidance_factor = None
 * (models/modules.py:643-670, 728-790: one feature grid per level, sliced at the pixel grid linspace x linspace with the image's
 * gray value as guidance, levels concatenated) -> affine_network -> the trainer's application with the residual
 * (models/trainers/scene_graph.py:99-106).  levels[l].grid is ONE image's grid [nch, gl, gy, gx] (the test branch's mean over
 * neighbour grids is linear: the caller averages the grids); rgb / out / v_out / v_rgb [H,W,3].
 * bwd ACCUMULATES the grid gradients into levels[l].v_grid (same shape; caller zeroes; may be NULL), writes v_rgb (both routes: the
 * application and the guidance; may be NULL) and the weight gradients as bds_mlp_head_bwd does.
 * Built for: one level with gl = 8 and 8 / 16 / 24 / 32 features, or the two levels {gl 1, 8 features} + {gl 8, 8 features}
 * (configs/omnire_neuralbilateral.yaml:246-252, omnire_ms_neuralbilateral.yaml:247-250), plus gl = 4 with 24 features and
 * {gl 1, 8} + {gl 4, 8} (the shapes of the reference-generated golden vectors), any gx, gy with at most 64 cell
 * boundaries per axis, W <= 4096, hidden 64: bds_neural_image_ok() != 0; otherwise BDS_EINVAL and the two-step form
 * (bds_bilagrid_slice_feat_image_* + bds_mlp_head_*) applies.  temp: bds_neural_image_bwd_temp_bytes(F) bytes. */
typedef struct {
  const float *grid;
  float *v_grid;
  int gx, gy, gl, nch;
} bds_feat_level;
int bds_neural_image_ok(int H, int W, int n_levels, const bds_feat_level *levels, int hidden);
size_t bds_neural_image_bwd_temp_bytes(int F);
int bds_neural_image_fwd(int H, int W, int n_levels, const bds_feat_level *levels, int hidden, const float *rgb, const float *w1,
                         const float *w2, const float *w3, int residual, float *out, bds_stream_t stream);
int bds_neural_image_bwd(int H, int W, int n_levels, const bds_feat_level *levels, int hidden, const float *rgb, const float *w1,
                         const float *w2, const float *w3, int residual, const float *v_out, float *v_rgb, float *v_w1, float *v_w2,
                         float *v_w3, int accumulate_w, void *temp, size_t temp_bytes, bds_stream_t stream);

/* ---- Deformation network of deformable Gaussians -----------------------------------------------------------------------------
 * ConditionalDeformNetwork / DeformNetwork (models/modules.py:925-1012, encoding `get_embedder` / `Embedder` :874-922) at the shipped
 * size: D 8, W 256, x_multires = t_multires 10, input_ch 3, embed_dim 16 (DeformableNodes, models/nodes/deformable.py:35-47, 49-143)
 * or 0 (DeformNetwork: models/gaussians/deformgs.py:62-72, 97-109); bds_deform_supported() != 0, anything else BDS_EINVAL.
 *   h0 = [emb(x) 63 | emb(t) 21 | cond E] (K0 = 84 + E), 8 x (Linear + ReLU), layer 5 reading [h0 | h4] (skips = [D // 2]),
 *   d_xyz = gaussian_warp(h), rotation = gaussian_rotation(h), scaling = gaussian_scaling(h).
 * x [N,3], t [N] (one time per point), cond [N,E] (NULL when E = 0), all float32 contiguous.  Weights in torch's [out, in] layout
 * (linear.{i}.weight [256, in_i]: in_0 = K0, in_5 = K0 + 256, else 256; heads [3|4|3, 256]); every weight 16-byte aligned.  A head
 * that is off has NULL weight and bias (ConditionalDeformNetwork deform_quat / deform_scale = False); gaussian_warp is always on.
 * fwd writes d_xyz [N,3] and rotation [N,4] / scaling [N,3] (each may be NULL).  One kernel on the FP32 matrix cores
 * (csrc/deform.hip): the hidden activations never reach memory.
 * bwd takes the output gradients (v_rotation / v_scaling may be NULL = zero), writes v_x [N,3], v_t [N], v_cond [N,E] (each may be
 * NULL) and the parameter gradients named in `grad` (each may be NULL; stored, or added to when accumulate != 0).  The forward is
 * recomputed chunk by chunk; temp: bds_deform_bwd_temp_bytes(N, E) bytes, 16-byte aligned (the chunk's activations / pre-activation
 * gradients and the per-tile partial weight gradients, summed in a fixed order: the result is deterministic, no atomics). */
typedef struct {
  const float *w[8], *b[8];                               /* linear.{i}.weight / .bias */
  const float *warp_w, *warp_b, *rot_w, *rot_b, *scale_w, *scale_b;
} bds_deform_net;
typedef struct {
  float *w[8], *b[8];
  float *warp_w, *warp_b, *rot_w, *rot_b, *scale_w, *scale_b;
} bds_deform_net_grad;
int bds_deform_supported(int D, int W, int x_multires, int t_multires, int input_ch, int embed_dim);
size_t bds_deform_bwd_temp_bytes(int64_t N, int embed_dim);
int bds_deform_fwd(int64_t N, int embed_dim, const float *x, const float *t, const float *cond, const bds_deform_net *net, float *d_xyz,
                   float *rotation, float *scaling, bds_stream_t stream);
int bds_deform_bwd(int64_t N, int embed_dim, const float *x, const float *t, const float *cond, const bds_deform_net *net,
                   const float *v_xyz, const float *v_rotation, const float *v_scaling, float *v_x, float *v_t, float *v_cond,
                   const bds_deform_net_grad *grad, int accumulate, void *temp, size_t temp_bytes, bds_stream_t stream);

/* ---- Pose transform of the node classes -------------------------------------------------------------------------------------------
 * RigidNodes.transform_means / transform_quats / get_pts_valid_mask and the activations of get_gaussians (models/nodes/rigid.py:28-32,
 * 385-493), the same for DeformableNodes (models/nodes/deformable.py:49-114, which calls them on the deformed means / quaternions).
 * Point p of instance i = point_ids[p] (int64 [N], the [N,1] column) at frame f = cur_frame, q_i = instances_quats[f,i] ([F,I,4]),
 * t_i = instances_trans[f,i] ([F,I,3]), instances_fv [F,I] (bool, one byte each):
 *   world_means[p] = R(q_i) means[p] + t_i                       (R: the normalising quat_to_rotmat of quat_act(q_i))
 *   world_quats[p] = n(quat_mult(n(q_i), n(quats[p])))          (n = quat_act, q / |q|: a zero quaternion gives NaN, as the reference)
 *   opacities[p]   = sigmoid(logits[p]) * instances_fv[f,i]
 * interpolate != 0: the test-set form (rigid.py:392-432), allowed only when cur_frame - 1 > 0 and cur_frame + 1 < F (else BDS_EINVAL):
 * the means' rotation is interpolate_quats(q[f-1], q[f+1]) (models/gaussians/basics.py:17-45) and the translation
 * (t[f-1] + t[f+1]) / 2 where instances_fv[f-1] & instances_fv[f+1], else frame f's; world_quats and the mask keep frame f.
 * An id outside [0, I) reads nothing: that point's outputs are NaN and bit 0 of *bad_ids (may be NULL) is raised, never cleared.
 * N = 0 launches nothing and writes nothing.  All arrays contiguous float32 unless said otherwise.
 * bwd (non-interpolated form only; the reference cannot differentiate the other): v_means [N,3], v_quats [N,4], v_logits [N] stored per
 * point (zero for an out-of-range id); v_instances_quats [F,I,4] / v_instances_trans [F,I,3] stored dense, zero outside frame f.  The
 * instance sums are reduced per wave in a fixed order into a [waves, I, 16] slab in temp (bds_node_pose_bwd_temp_bytes(N, I) bytes,
 * 16-byte aligned) and summed per instance in a fixed order: the result is deterministic, no float atomics. */
size_t bds_node_pose_bwd_temp_bytes(int64_t N, int I);
int bds_node_pose_fwd(int64_t N, int F, int I, int cur_frame, int interpolate, const float *means, const float *quats, const float *logits,
                      const int64_t *point_ids, const float *instances_quats, const float *instances_trans, const uint8_t *instances_fv,
                      float *world_means, float *world_quats, float *opacities, uint32_t *bad_ids, bds_stream_t stream);
int bds_node_pose_bwd(int64_t N, int F, int I, int cur_frame, const float *means, const float *quats, const float *logits,
                      const int64_t *point_ids, const float *instances_quats, const uint8_t *instances_fv, const float *v_world_means,
                      const float *v_world_quats, const float *v_opacities, float *v_means, float *v_quats, float *v_logits,
                      float *v_instances_quats, float *v_instances_trans, void *temp, size_t temp_bytes, bds_stream_t stream);

/* ---- Pose chain and skinning of the SMPL nodes -------------------------------------------------------------------------------------
 * SMPLNodes.transform_means_and_quats / transform_means (models/nodes/smpl.py:203-341) with SMPLTemplate.forward
 * (models/human_body.py:158-180), batch_rigid_transform (third_party/smplx/smplx/lbs.py:362-418) and VoxelDeformer.forward
 * (models/modules.py:1168-1188).  Instance i owns the rows [i V, (i+1) V) of means [I V,3] and quats [I V,4] (raw).  Per instance:
 * root_quats [I,1,4] and body_quats [I,23,4] (the current frame's raw rows), trans [I,3], present [I] (one byte each),
 * J_canonical [I,24,3], A0_inv [I,24,4,4]; parents: 24 int32 on the HOST, parents[0] unused, 0 <= parents[j] < j (else BDS_EINVAL,
 * nothing launched).  The weights: voxel_base and voxel_corr (may be NULL) [I,24,d,h,w] with offset [I,1,3], scale [I,1,1], ratio and
 * ratio_dim (0..2: the component of the normalised coordinate that ratio multiplies); or, with voxel_base NULL, the fixed W [I,V,24].
 *   theta = normalise(cat(root, body)); R_j = quaternion_to_matrix(theta_j) (pytorch3d, 2 / |q|^2); the chain of
 *   batch_rigid_transform with its rel_transforms column, times A0_inv: A [I,24,3,4] (rows 0..2; stored for the backward)
 *   w = trilinear sample of voxel_base + voxel_corr at (x - offset) / scale (component ratio_dim times ratio), align_corners, border
 *   T = sum_j w_j A_j; world_means = T.R x + T.t + trans; world_quats = quat_mult(n(matrix_to_quaternion(T.R)), n(quats))
 *   (pytorch3d's matrix_to_quaternion on the non-orthogonal blend: largest q_abs, / (2 max(q_abs, 0.1)), sign to w >= 0).
 * An absent instance (present[i] == 0): world_means = trans[i], world_quats = (1,0,0,0), A = 0.  world_quats NULL: the ball form
 * (means only; quats may be NULL).
 * bwd: v_means (the direct term and the one through the sampling coordinate; a clamped axis has none), v_quats (NULL iff
 * v_world_quats is), v_root_quats [I,1,4] / v_body_quats [I,23,4] (to the RAW quaternions), v_trans [I,3], v_voxel_corr [I,24,d,h,w]
 * (may be NULL; zeroed here, then float atomics: its summation order is unspecified).  An absent instance: v_trans[i] = the sum of its
 * rows' v_world_means, every other gradient of it zero.  Pose and translation gradients are summed per workgroup and then per
 * instance in a fixed order in temp (bds_smpl_skin_bwd_temp_bytes(I, V) bytes, 16-byte aligned): deterministic. */
size_t bds_smpl_skin_bwd_temp_bytes(int I, int V);
int bds_smpl_skin_fwd(int I, int V, const float *means, const float *quats, const float *root_quats, const float *body_quats,
                      const float *trans, const uint8_t *present, const float *J_canonical, const float *A0_inv, const int32_t *parents,
                      const float *voxel_base, const float *voxel_corr, const float *W, int d, int h, int w, const float *offset,
                      const float *scale, float ratio, int ratio_dim, float *world_means, float *world_quats, float *A,
                      bds_stream_t stream);
int bds_smpl_skin_bwd(int I, int V, const float *means, const float *quats, const float *root_quats, const float *body_quats,
                      const uint8_t *present, const float *J_canonical, const float *A0_inv, const int32_t *parents,
                      const float *voxel_base, const float *voxel_corr, const float *W, int d, int h, int w, const float *offset,
                      const float *scale, float ratio, int ratio_dim, const float *A, const float *v_world_means,
                      const float *v_world_quats, float *v_means, float *v_quats, float *v_root_quats, float *v_body_quats,
                      float *v_trans, float *v_voxel_corr, void *temp, size_t temp_bytes, bds_stream_t stream);

/* ---- The SMPL nodes' every-step regularisers ---------------------------------------------------------------------------------------
 * knn_reg of SMPLNodes.compute_reg_loss (models/nodes/smpl.py:462-503).  nn_ind [I,V,K] int32: within-instance indices in [0,V) (the
 * query itself and repeats allowed; the caller validates them -- an index outside the range reads row 0), 2 <= K <= 32; present [I]
 * (one byte each: instances_fv[cur_frame]).  Five attribute groups, each pointer may be NULL (a frozen group: term 0, no gradient):
 * features_dc [I V,3], features_rest [I V,c_rest] (c_rest 9, 24 or 45), opacities [I V,1] (raw; sigmoid inside), scales [I V,s_dim]
 * (raw; exp inside; s_dim 1 or 3), quats [I V,4] (raw).
 *   terms[g] = mean over (present instance, point, channel of g) of the unbiased std over the K gathered values of that channel
 * (:472, :480, :487, :495, :502; two passes: the mean as v_0 + sum(v_k - v_0) / K, then the squared deviations), in the order dc,
 * rest, opacity, scales, quats; 0 with no instance present.  One launch over (row, channel) of the live groups (mean and
 * rstd = 1 / ((K-1) std), 0 where std == 0, stored per (row, channel) of the `channels` live ones: [I V, channels] each, kept for
 * the backward) and a one-workgroup finish that sums the workgroups' rows of temp (bds_smpl_knn_reg_temp_bytes bytes) in a fixed
 * order and leaves norm[5] = 1 / (present V C_g), formed on the device.
 * bwd: ONE launch in gather form.  rev_offsets [I,V+1] / rev_edges [I,V K] (int32): the (point K + slot) pairs that list each row,
 * ascending; row r of group g receives v_terms[g] norm[g] sum_edges (a_r - mean_p) rstd_p, times the activation's derivative
 * (gradients to the RAW parameters), summed in list order: no atomics, bit-identical run to run.  Rows of absent instances and rows
 * nobody lists are written zeros.  v_<group> NULL exactly where <group> is. */
size_t bds_smpl_knn_reg_temp_bytes(int I, int V, int channels);
int bds_smpl_knn_reg_fwd(int I, int V, int K, const int32_t *nn_ind, const uint8_t *present, const float *features_dc,
                         const float *features_rest, int c_rest, const float *opacities, const float *scales, int s_dim,
                         const float *quats, float *terms, float *norm, float *mean, float *rstd, void *temp, size_t temp_bytes,
                         bds_stream_t stream);
int bds_smpl_knn_reg_bwd(int I, int V, int K, const int32_t *rev_offsets, const int32_t *rev_edges, const uint8_t *present,
                         const float *features_dc, const float *features_rest, int c_rest, const float *opacities, const float *scales,
                         int s_dim, const float *quats, const float *mean, const float *rstd, const float *norm, const float *v_terms,
                         float *v_features_dc, float *v_features_rest, float *v_opacities, float *v_scales, float *v_quats,
                         bds_stream_t stream);

/* voxel_deformer_reg of SMPLNodes.compute_reg_loss (models/nodes/smpl.py:448-459): VoxelDeformer.get_tv and get_mag
 * (models/modules.py:1139-1166) of one field [I,J,D,H,W], 1 <= J <= 64, D, H, W >= 2 (else BDS_EINVAL: the reference's mean over an
 * empty slice is NaN).
 *   terms[0] = (mean|x[d+1] - x| + mean|x[h+1] - x| + mean|x[w+1] - x|) / 3, each mean over its own count (:1148-1151)
 *   terms[1] = mean over [I,D,H,W] of the 2-norm over J (:1166)
 * One pass, a thread per voxel walking J; rnorm [I,D,H,W] = 1 / norm (0 for the zero vector) is kept for the backward; the
 * workgroups' rows of temp (bds_voxel_reg_temp_bytes bytes) are summed in a fixed order by a one-workgroup finish.
 * bwd: one pass in gather form, v_field[e] = v_terms[0] / 3 (the signs of e's up to six differences over their counts; sign(0) = 0)
 * + v_terms[1] x rnorm / (I D H W): every element written, no atomics, bit-identical run to run. */
size_t bds_voxel_reg_temp_bytes(int I, int D, int H, int W);
int bds_voxel_reg_fwd(int I, int J, int D, int H, int W, const float *field, float *terms, float *rnorm, void *temp, size_t temp_bytes,
                      bds_stream_t stream);
int bds_voxel_reg_bwd(int I, int J, int D, int H, int W, const float *field, const float *rnorm, const float *v_terms, float *v_field,
                      bds_stream_t stream);

/* Time transform of the periodic-vibration Gaussians: PeriodicVibrationGaussians.get_gaussians (models/gaussians/pvg.py:374-425) with
 * get_marginal_t (:81), temporal_means (:65-73), temporal_opacities (:75-78) and velocity / rho (:83-88), as three forward launches and
 * one backward launch.  Raw parameters, contiguous float32: means [N,3], velocity [N,3], taus [N], betas [N], logits [N] (the [N,1]
 * columns), log_scales [N,3], quats [N,4], features_dc [N,3], features_rest [N,K-1,3] (may be NULL for K = 1), cam_pos [3].  With
 * d = tau - cur_time, s_t = exp(beta), a = 2 pi / T (T: ctrl_cfg.cycle_length, a double as in the reference: a is formed in double
 * and rounded to float32 once, where the Python scalar meets the float32 tensor; cur_time and delta_t arrive rounded the same way):
 *   marg = exp(-0.5 d^2 / s_t^2); a row is KEPT when marg > 0.05 in float32 (a NaN tau / beta drops it, as the reference's comparison)
 *   mean' = mean + velocity sin((cur_time - tau) a) / a, + velocity exp(-0.5 s_t / T) delta_t when in_smooth
 *   opacity = sigmoid(logit) marg, scale = exp(log_scale), quat = q / |q|
 *   rgb = clamp(SH(degrees_to_use, normalise(mean' - cam_pos)) + 0.5, 0, 1); K = 1 (the class's sh_degree == 0): sigmoid(features_dc)
 * fwd: the kept rows' outputs COMPACTED in the original order (x[filter_mask]) at the front of out_* (each allocated for N rows;
 * out_sh_raw [N,3]: the colour before + 0.5 and the clamp -- band 0 itself for K = 1 -- for the backward), filter_mask [N] one byte per
 * row.  temp (bds_pvg_temp_bytes(N) bytes, 16-byte aligned) starts with uint32 {M, flags, 0, 0}: M = rows kept, flags bit 2 i = a NaN,
 * bit 2 i + 1 = an Inf among the kept rows of tensor i (means, opacities, rgbs, scales, quats: the order of :419-423); behind it the
 * exclusive scan of the kept rows per 256-row block, which bwd reads again.  One read of the header gives the host M and the flags.
 * bwd (M as read from the header; the same scalars, parameters, filter_mask, temp, out_means and out_sh_raw as fwd left them):
 * v_out_* [M,.] are read by rank; EVERY row of v_means [N,3] v_velocity [N,3] v_taus [N] v_betas [N] v_logits [N] v_log_scales [N,3]
 * v_quats [N,4] v_features_dc [N,3] v_features_rest [N,K-1,3] is stored, zeros for a dropped row (no memset needed).  The view
 * direction is detached, the clamp passes the gradient on the closed interval.  No atomics: bit-identical run to run.
 * BDS_EINVAL before any launch: N < 0 or > INT32_MAX, K not in {1, 4, 9, 16}, (degrees_to_use + 1)^2 > K, T <= 0, a NULL array with
 * N > 0, a misaligned or short temp.  N = 0 launches nothing. */
size_t bds_pvg_temp_bytes(int64_t N);
int bds_pvg_fwd(int64_t N, int K, int degrees_to_use, float cur_time, float delta_t, int in_smooth, double T, const float *means,
                const float *velocity, const float *taus, const float *betas, const float *logits, const float *log_scales,
                const float *quats, const float *features_dc, const float *features_rest, const float *cam_pos, float *out_means,
                float *out_opacities, float *out_rgbs, float *out_scales, float *out_quats, float *out_sh_raw, uint8_t *filter_mask,
                void *temp, size_t temp_bytes, bds_stream_t stream);
int bds_pvg_bwd(int64_t N, int64_t M, int K, int degrees_to_use, float cur_time, float delta_t, int in_smooth, double T,
                const float *velocity, const float *taus, const float *betas, const float *logits, const float *log_scales,
                const float *quats, const float *cam_pos, const uint8_t *filter_mask, const void *temp, size_t temp_bytes,
                const float *out_means, const float *out_sh_raw, const float *v_out_means, const float *v_out_opacities,
                const float *v_out_rgbs, const float *v_out_scales, const float *v_out_quats, float *v_means, float *v_velocity,
                float *v_taus, float *v_betas, float *v_logits, float *v_log_scales, float *v_quats, float *v_features_dc,
                float *v_features_rest, bds_stream_t stream);

/* Evaluation image metrics of one frame: render_images' scoring (models/video_utils.py:29-44,273-361), i.e. compute_psnr and
 * skimage.metrics.structural_similarity(data_range=1.0, channel_axis=-1) -- 7x7 uniform window, sample covariance (cov_norm 49/48),
 * scipy's mode="reflect" borders, C1 = 0.01^2, C2 = 0.03^2, the mean taken over rows / columns 3 .. H-4 / 3 .. W-4 per channel and
 * then over the channels -- and both under up to four pixel masks, in two launches and without a host wait.  pred, gt: [H,W,3]
 * float32.  mask0..3: [H,W] or NULL (slot unused); mask_kind 0 = one byte per pixel (uint8 / bool), 1 = float32, non-zero = true as
 * astype(bool) reads it; bit s of invert_bits scores the pixels where slot s is FALSE (the sky mask, :292).  A slot's PSNR is
 * compute_psnr over its pixels' three channels, its SSIM the mean of the UNCROPPED map over them (S[mask].mean(), :306).
 * ssim_map: NULL or [H,W,3] float32, the map of full=True.  out: BDS_IMAGE_METRICS_ROW doubles {psnr, ssim, (psnr, ssim) of slot
 * 0..3, valid of slot 0..3}: valid = 1.0 when the slot scored at least one pixel, else 0.0 with NaN values; psnr = -10 log10(mse) is
 * +inf for identical images.  ws: bds_image_metrics_workspace_bytes(H, W) bytes, 16-byte aligned (one row of partial sums per 16x16
 * tile, added in a fixed order in double: no atomics, bit-identical run to run).  This is NOT the training loss's SSIM (bds_ssim_fwd:
 * 11x11 Gaussian window, VALID region).  BDS_EINVAL before any launch: H or W < 7 (skimage raises there too) or > 2^19, a NULL pred /
 * gt / out / ws, an invert bit on a NULL slot, a misaligned pointer; BDS_EWORKSPACE: ws too small (the size query answers 0 for a
 * refused shape). */
#define BDS_IMAGE_METRICS_ROW 14
size_t bds_image_metrics_workspace_bytes(int H, int W);
int bds_image_metrics(int H, int W, const float *pred, const float *gt, const void *mask0, const void *mask1, const void *mask2,
                      const void *mask3, int invert_bits, int mask_kind, float *ssim_map, double *out, void *ws, size_t ws_bytes,
                      bds_stream_t stream);

/* Evaluation geometry metrics of one frame: render_images' geometry block (models/video_utils.py:363-536) over
 * utils/chamfer_distance.py:34-75, without pytorch3d and without a host wait.  pred (the render's expected depth), gt (the lidar depth
 * map): [H,W] float32.  egocar, mask0..3 (sky, dynamic, human, vehicle): [H,W] or NULL (all false); mask_kind as bds_image_metrics.
 * K: the row-major 3x3 intrinsics, c2w: the row-major 4x4 camera-to-world, both float32 ON THE DEVICE.
 *   valid = gt > 0 and not egocar and 0.01 < gt < 80 and 1e-4 < pred < 80; pixel (v,u) with depth z -> ((u-cx) z/fx, (v-cy) z/fy, z, 1)
 *   through c2w in float32; both clouds use the same valid pixels (n points each, row-major order).
 *   cham_pred[i]: the SQUARED distance from pred point i to its nearest lidar point, cham_gt the converse (knn_points(norm=2, K=1)
 *   .dists), from coordinate differences in float32.  A trimmed mean at q is the mean over the k = int(n*q) smallest (k as Python
 *   forms it; k = 0: NaN).  A class holds the valid pixels of its mask, the background those of none of the four.
 * row_out: BDS_GEOMETRY_METRICS_ROW doubles (8-byte aligned):
 *   [0..3]   chamfer, chamfer_99, _97, _95: mean (trimmed mean) of cham_pred + that of cham_gt
 *   [4..7]   depth_err = sqrt(mean(err^2)), depth_err_rmse_99, _97, _95 over the k smallest |err|, err = pred - gt
 *   [8]      depth_err_median_squared: the element of rank (n-1)/2 of err^2 (torch's lower median)
 *   [9..13]  chamfer of sky, dynamic, human, vehicle, background: the two means within the class, summed; NaN for an empty class
 *   [14]     n;  [15..19] the classes' point counts
 *   [20..23] mean, _99, _97, _95 of cham_pred;  [24..27] of cham_gt;  [28..31] of |err|
 * n = 0 gives NaN in every value.  dist_pred, dist_gt: both NULL, or [H*W] float32 whose first n entries receive cham_pred / cham_gt.
 * ws: bds_geometry_metrics_workspace_bytes(H, W) bytes, 16-byte aligned: the capacity is H*W points (about 57 bytes per pixel); the
 * launches are sized by it and leave early on the device's counts.  The pair loop takes BDS_GEOMETRY_QUERY_BLOCK queries per
 * workgroup against LDS tiles of BDS_GEOMETRY_TARGET_TILE targets.  Every sum is taken in double in a fixed order: bit-identical run
 * to run.  BDS_EINVAL before any launch: H or W < 1 or H*W > 2^24, a NULL pred / gt / K / c2w / row_out / ws, one distance array
 * without the other, a misaligned pointer, a mask_kind other than 0 / 1; BDS_EWORKSPACE: ws too small (the size query answers 0 for a
 * refused shape).
 * bds_depth_unproject: depth_map_to_point_cloud (chamfer_distance.py:54-75).  points [H*W,3]: the first *count rows receive the world
 * points of the pixels where mask (NULL: every pixel) is non-zero, in row-major pixel order; count: int64 on the device.  Same
 * workspace size and checks.
 * bds_chamfer_nn: x [P1,3], y [P2,3] float32 -> dist_x [P1], dist_y [P2]: per point the squared Euclidean distance (norm 2) or the sum
 * of absolute differences (norm 1) to the nearest point of the other cloud (+inf when that cloud is empty).  BDS_EINVAL: a negative
 * count or one above INT32_MAX, a norm other than 1 / 2, a NULL or misaligned array of a non-empty cloud. */
#define BDS_GEOMETRY_METRICS_ROW 32
#define BDS_GEOMETRY_QUERY_BLOCK 512
#define BDS_GEOMETRY_TARGET_TILE 512
size_t bds_geometry_metrics_workspace_bytes(int H, int W);
int bds_geometry_metrics(int H, int W, const float *pred, const float *gt, const void *egocar, const void *mask0, const void *mask1,
                         const void *mask2, const void *mask3, int mask_kind, const float *K, const float *c2w, double *row_out,
                         float *dist_pred, float *dist_gt, void *ws, size_t ws_bytes, bds_stream_t stream);
int bds_depth_unproject(int H, int W, const float *depth, const void *mask, int mask_kind, const float *K, const float *c2w,
                        float *points, int64_t *count, void *ws, size_t ws_bytes, bds_stream_t stream);
int bds_chamfer_nn(int64_t P1, int64_t P2, const float *x, const float *y, int norm, float *dist_x, float *dist_y, bds_stream_t stream);

/* Scene initialisation: the exact K nearest neighbours of every point of a cloud among the OTHER points of the same cloud, and the
 * initial log-scales from them -- k_nearest_sklearn (models/gaussians/basics.py:208-224: a kd-tree on the host over n_neighbors =
 * k + 1, first column dropped) as create_from_pcd (models/gaussians/vanilla.py:79-105) and the rigid nodes' initialiser
 * (models/nodes/rigid.py:113-120) call it, without the host.  x: [N,3] float32, every coordinate FINITE (the entry does not check;
 * a caller must -- bds_nonfinite_flags).  K: 1..BDS_KNN_MAX_K.
 *   dist [N,K]: the Euclidean distances, ascending, in the rows' original order: sqrt of (dx*dx + dy*dy) + dz*dz from the float32
 *   coordinate differences, every operation rounded on its own.  idx [N,K] int32 or NULL: the neighbours' rows.  A point is never
 *   its own neighbour (excluded by row, not by distance: a duplicate of a point is its neighbour at distance 0).  Candidates are
 *   ordered by (d2, row), so the result does not depend on the order of evaluation: bit-identical run to run.
 *   log_scales [N,S] or NULL, S 1..3: every column log(min(max(mean of the K distances, clamp_lo), clamp_hi)) -- clamp 0, +inf passes
 *   the mean through (a mean of 0 gives -inf, as torch.log in vanilla.py:85-92); rigid.py:118 clamps to 0.002, 100.
 * Method (csrc/knn.hip): a uniform grid (at most max(1, 2 N) cells, chosen on the device) over the cloud's box with at most N / 128
 * points trimmed beyond each face (two histogram passes; the border cells hold what lies beyond, and exactness does not depend on the
 * box), a counting sort of 16-byte records by cell, one lane per record walking the rings of cells r = 0..BDS_KNN_RING_MAX around
 * its own with a conservative
 * termination test, and an exact brute-force pass (BDS_KNN_QUERY_BLOCK queries per workgroup against LDS tiles of
 * BDS_KNN_TARGET_TILE records) for the queries the rings leave unresolved.  Eleven launches, no host wait, no allocation.
 * ws: bds_knn_workspace_bytes(N) bytes (about 28 per point), 16-byte aligned.  It starts with the stats block, BDS_KNN_STATS_WORDS
 * 32-bit words, valid behind the call: [BDS_KNN_STAT_EDGE] the cell edge (float), [+1] its inverse, [+2] the margin's slack,
 * [BDS_KNN_STAT_DIMS..+2] the cells per axis (int), [BDS_KNN_STAT_UNRESOLVED] the queries the fallback took (uint),
 * [BDS_KNN_STAT_LO..+2] / [BDS_KNN_STAT_HI..+2] the grid's box (float), [BDS_KNN_STAT_CELLS] the cells in all (uint),
 * [BDS_KNN_STAT_CLOUD_LO..+2] / [BDS_KNN_STAT_CLOUD_HI..+2] the cloud's box (float).
 * BDS_EINVAL before any launch: K outside 1..BDS_KNN_MAX_K; N < K + 1 or N > BDS_KNN_MAX_POINTS; a NULL x, dist or ws; log_scales
 * with S outside 1..3, clamp_lo > clamp_hi or a NaN clamp; a pointer not aligned to 4 bytes (ws: 16).  BDS_EWORKSPACE: ws too small
 * (the size query answers 0 for N < 2 or N > BDS_KNN_MAX_POINTS). */
#define BDS_KNN_MAX_K 8
#define BDS_KNN_MAX_POINTS 1073741824
#define BDS_KNN_QUERY_BLOCK 256
#define BDS_KNN_TARGET_TILE 512
#define BDS_KNN_RING_MAX 2
#define BDS_KNN_STATS_WORDS 32
#define BDS_KNN_STAT_EDGE 0
#define BDS_KNN_STAT_DIMS 3
#define BDS_KNN_STAT_UNRESOLVED 6
#define BDS_KNN_STAT_LO 7
#define BDS_KNN_STAT_HI 10
#define BDS_KNN_STAT_CELLS 13
#define BDS_KNN_STAT_CLOUD_LO 14
#define BDS_KNN_STAT_CLOUD_HI 17
size_t bds_knn_workspace_bytes(int64_t N);
int bds_knn_self(int64_t N, const float *x, int K, float *dist, int32_t *idx, float *log_scales, int S, float clamp_lo, float clamp_hi,
                 void *ws, size_t ws_bytes, bds_stream_t stream);

/* Exact K nearest rows of p2[b] for every row of p1[b], batched, forward only: pytorch3d.ops.knn_points as the reference calls it --
 * models/modules.py:1199 (VoxelDeformer._query_weights_smpl: K = 30 of the template's 6890 vertices for each of 16*64*64 voxel
 * centres per human), models/nodes/smpl.py:186 (update_knn: a batch of clouds against themselves, K = 3, the query included) and
 * utils/chamfer_distance.py:45-46 (K = 1) -- with the inverse-distance blend of modules.py:1200-1206 as an epilogue.  One launch, no
 * workspace, no host wait (csrc/knn_cross.hip).  p1 [B,P1,3], p2 [B,P2,3] float32; the entry does NOT check that the coordinates are
 * finite (pytorch3d does not either): a NaN coordinate makes a NaN value, which never enters a list.
 *   value   norm 2: the SQUARED distance (dx*dx + dy*dy) + dz*dz from the float32 coordinate differences, every operation rounded on
 *           its own (no fused multiply-add); norm 1: (|dx| + |dy|) + |dz|.
 *   order   ascending; candidates are ordered by (value, row of p2), so the row decides ties, the result does not depend on the order
 *           of evaluation and is bit-identical run to run.  The query is NOT excluded: a cloud against itself finds each point first.
 *   lengths len1 / len2 [B] int64 on the device or NULL (every cloud full), clamped to 0..P1 / 0..P2 on the device.  Only the first
 *           len2[b] rows of p2[b] are candidates; rows of p1[b] at or beyond len1[b], and the slots len2[b]..K-1 of every row, hold
 *           dists = 0 and idx = 0 (pytorch3d's padding).  Every element of every output is written.
 *   dists [B,P1,K] float32 or NULL, idx [B,P1,K] int64 or NULL.
 *   blend [B,P1,J] float32 or NULL, together with feat [B,P2,J] (both or neither; norm 2 only; J 1..BDS_KNN_CROSS_MAX_J;
 *           0 < clamp_lo <= clamp_hi): w_k = 1 / min(max(sqrt(d2_k), clamp_lo), clamp_hi) over the slots that hold a neighbour,
 *           blend[j] = sum_k (w_k / sum w) * feat[idx_k][j], k ascending; a row without a neighbour gets zeros.  dists and idx may
 *           then both be NULL.
 * BDS_KNN_CROSS_QUERY_BLOCK queries of one cloud per workgroup, the candidates staged through LDS in tiles of
 * BDS_KNN_CROSS_TARGET_TILE records.  B, P1 or P2 equal to 0 is valid: nothing is launched when B * P1 = 0, and everything is padding
 * when P2 = 0.
 * BDS_EINVAL before any launch: K outside 1..BDS_KNN_CROSS_MAX_K; norm outside {1, 2}; a negative size, P2 >= 2^31 - 1 or more than
 * 2^31 - 1 workgroups; a NULL p1 / p2 that has elements; dists, idx and blend all NULL; feat without blend or the converse; a blend
 * with norm 1, J out of range, P2 * J above 2^29 or a clamp that is not 0 < lo <= hi; a float pointer not aligned to 4 bytes, idx / len1 / len2 to 8. */
#define BDS_KNN_CROSS_MAX_K 32
#define BDS_KNN_CROSS_MAX_J 64
#define BDS_KNN_CROSS_QUERY_BLOCK 256
#define BDS_KNN_CROSS_TARGET_TILE 512
int bds_cross_knn(int B, int64_t P1, int64_t P2, const float *p1, const float *p2, const int64_t *len1, const int64_t *len2, int K, int norm,
                  float *dists, int64_t *idx, const float *feat, int J, float clamp_lo, float clamp_hi, float *blend, bds_stream_t stream);

/* Lidar scene preparation: what DrivingDataset makes of the lidar before step 0, and the sparse depth map's downsampler of every
 * coarse-to-fine step.  points: [N,3] float32, every coordinate FINITE (the entries do not check; a caller must --
 * bds_nonfinite_flags).  Matrices are row-major float32 ON THE DEVICE.  One thread per point (per pixel / output cell where said); the
 * per-view and per-box tables go through LDS in chunks of BDS_LIDAR_VIEW_CHUNK / BDS_LIDAR_BOX_CHUNK.  No float atomics anywhere:
 * every output is bit-identical run to run.  Rows, pixels and records are 32-bit: N, V*H*W, B*H*W and B*Ho*Wo at most 2^31 - 257.
 *
 * bds_lidar_project -- project_lidar_pts_on_images (datasets/driving_dataset.py:644-727) for V views of one camera (common W, H).
 *   lidar2img [V,3,4]: the first three rows of pad(K) @ inverse(c2w) (:681-685).  ranges [V,2] int64: view v takes the rows
 *   [begin, end) of points (its lidar sweep), clamped to [0, N].  Per point and view: q = M[:, :3] p + M[:, 3] as
 *   ((m0 x + m1 y) + m2 z) + m3 without fused multiply-add, z = q.z, u = q.x / (z + 1e-6f), v = q.y / (z + 1e-6f); valid iff
 *   0 <= u < W and 0 <= v < H and z > 0 (:690-698); pixel ((int)v, (int)u) (:704-706).
 *   winner [V,H,W] int32: per pixel the HIGHEST valid row, -1 where none landed -- what the reference's index_put_ with duplicate
 *   indices gives on the host (the last write wins) and leaves unspecified on a GPU.  Three passes: an integer atomicMax of the row,
 *   a per-pixel pass that writes depth [V,H,W] = the winner's z (0 where empty), a per-point pass that writes pix [N] (the linear
 *   index (v*H + y)*W + x of the point's pixel in the LAST view that sees it, else -1), SETS visible [N] to 1 where pix >= 0 (other
 *   bytes keep their value: launches accumulate, :714) and, with images [V,H,W,3] and colors [N,3] (both or neither), copies the
 *   image's pixel to colors for every valid point, winner or not (:717-720; other rows keep their value).
 *   V = 0 and N = 0: nothing to do.  V > 0, N = 0: winner = -1, depth = 0.
 * bds_lidar_visible -- check_pts_visibility (:576-603): visible [N] = 1 where the valid test above holds in any of V views, else 0.
 *   sizes [V,2] int32: (W, H) of each view.  V = 0 writes zeros.
 * bds_lidar_points_in_boxes* -- the oriented-box test of get_init_objects (:341-354) and filter_pts_in_boxes (:521-536) for B boxes.
 *   w2o [B,3,4]: the first three rows of inverse(o2w); half [B,3]: o_size / 2; ranges [B,2] int64 or NULL: the rows a box tests (its
 *   frame's sweep; NULL: every row).  o = w2o [p;1] as above; inside iff -half < o < half on every axis, strictly.  chunk: boxes per
 *   LDS stage, 1..BDS_LIDAR_BOX_CHUNK (the product passes BDS_LIDAR_BOX_CHUNK; tests pass less to cross stages with few boxes).
 *   Mask form (bds_lidar_points_in_boxes): inside [N] = 1 where any box holds the point, else 0 (B = 0: zeros).
 *   Emit form: bds_lidar_points_in_boxes_count writes per point the number of boxes that hold it and scans them (ws:
 *   bds_lidar_boxes_workspace_bytes(N) bytes, 16-byte aligned) and writes *total (int64, device), the number of records;
 *   bds_lidar_points_in_boxes_emit, given the SAME arguments and that workspace, writes record r < capacity as rec_ids [r] =
 *   (instance, frame, row) from ids [B,2] int32 = (instance, frame) and rec_xyz [r] = o, ordered by (row, box): a point inside two
 *   boxes gives two records.  Records at or past capacity are dropped (the caller reads *total to size the arrays).
 * bds_lidar_depth_downsample -- sparse_lidar_map_downsampler (datasets/base/pixel_source.py:77-92) for B maps [B,H,W] -> [B,Ho,Wo]:
 *   output cell (i,j) covers rows [floor(i H / Ho), ceil((i+1) H / Ho)) and columns likewise (F.interpolate(mode="area")); with sum
 *   over every value of the window in row-major order, cnt the number of values > 1e-3 and kh x kw the window:
 *   ((sum / kh) / kw) / ((cnt / kh) / kw) where cnt > 0, else 0 -- the reference's order of divisions on the host.  Ho, Wo may exceed H, W (a scale
 *   factor above 1: the same windows, single pixels or overlapping).
 * All: 0 for an empty input; BDS_EINVAL before any launch for a negative or too large count, a NULL or misaligned array that the
 * call would read or write, images without colors or the converse, a chunk outside its range; BDS_EWORKSPACE: ws too small (the size
 * query answers 0 for N < 1 or too large). */
#define BDS_LIDAR_VIEW_CHUNK 64
#define BDS_LIDAR_BOX_CHUNK 128
int bds_lidar_project(int V, int W, int H, int64_t N, const float *points, const float *lidar2img, const int64_t *ranges,
                      const float *images, int32_t *winner, float *depth, int32_t *pix, uint8_t *visible, float *colors,
                      bds_stream_t stream);
int bds_lidar_visible(int64_t N, const float *points, int V, const float *lidar2img, const int32_t *sizes, uint8_t *visible,
                      bds_stream_t stream);
int bds_lidar_points_in_boxes(int64_t N, const float *points, int B, const float *w2o, const float *half, const int64_t *ranges,
                              int chunk, uint8_t *inside, bds_stream_t stream);
size_t bds_lidar_boxes_workspace_bytes(int64_t N);
int bds_lidar_points_in_boxes_count(int64_t N, const float *points, int B, const float *w2o, const float *half, const int64_t *ranges,
                                    int chunk, int64_t *total, void *ws, size_t ws_bytes, bds_stream_t stream);
int bds_lidar_points_in_boxes_emit(int64_t N, const float *points, int B, const float *w2o, const float *half, const int64_t *ranges,
                                   const int32_t *ids, int chunk, const void *ws, size_t ws_bytes, int64_t capacity, int32_t *rec_ids,
                                   float *rec_xyz, bds_stream_t stream);
int bds_lidar_depth_downsample(int B, int H, int W, int Ho, int Wo, const float *in, float *out, bds_stream_t stream);

/* Pseudo-lidar generation: a rendered depth map (or a cloud) turned into a simulated lidar sweep -- every pixel unprojected, moved
 * into the lidar's frame, cropped to the sensor's box and binned into an H x W angular map of beams, the occupied beams returned in
 * beam order.  Where several pixels (rows) fall into one beam the HIGHEST linear pixel index v*Wi + u (the highest row) wins: what
 * the reference's numpy assignment with duplicate indices gives (the last write).  Two launches per call: an integer atomicMax of
 * the index into winner [C,H,W] (reset to -1 by the entry, on the stream), then one workgroup per camera that ranks the occupied
 * cells of the kept rows (row % slice == 0) in cell order and writes, at its rank r < counts[c], the winner's coordinates --
 * recomputed by the same function, the same bits -- to points [c, r] and, with source != NULL, its index to source [c, r].  Rows at
 * and past counts[c] are left untouched.  cap = ceil(H / slice) * W rows per camera.  No float atomics: bit-identical run to run.
 *
 * beams: BDS_PSEUDO_LIDAR_BEAMS doubles ON THE DEVICE, formed by the caller with the reference's own expressions:
 *   [0] rad(45), [1] dphi = rad(90 / W), [2] theta0, [3] fov_up, [4] dtheta, [5..10] the crop x0 x1 y0 y1 z0 z1, [11] max_depth.
 *   The angles are taken in double from the widened float32 coordinates (the reference's numpy part is float64):
 *   d = sqrt((x x + y y) + z z), r = sqrt(x x + y y), each 1e-6 where 0; column = trunc((rad45 - asin(y / r)) / dphi) clamped to
 *   [0, W-1] (no point is dropped: beyond +-45 degrees it lands in an edge column).
 *   mode BDS_PSEUDO_LIDAR_VERTICAL (pto_ang_map_vertical): theta = asin(z / d), kept iff theta0 <= theta <= fov_up (theta0 =
 *   fov_down, dtheta = (fov_up - fov_down) / H), row = trunc((theta - theta0) / dtheta) clamped to [0, H-1].
 *   mode BDS_PSEUDO_LIDAR_CLASSIC (pto_ang_map): row = trunc((theta0 - asin(z / d)) / dtheta) clamped, no filter (theta0 = rad(2),
 *   dtheta = rad(0.4 * 64 / H)).
 * bds_pseudo_lidar_from_depth -- depth_map_to_lidar_points (generate_lidar/generate_lidar_from_depth.py:95-162) for the C cameras of a
 *   frame in one call.  depth [C,Hi,Wi]; cams [C,16] float32: fx fy cx cy (after the division by downscale_when_loading) and the
 *   [3,4] camera-to-lidar matrix inverse(lidar_to_world) @ cam_to_world, formed in double and rounded once (the reference takes two
 *   float32 products through world coordinates).  Per pixel: valid iff d > 0 && d < max_depth (a NaN is not); xc = ((u - cx) d) / fx,
 *   yc = ((v - cy) d) / fy, zc = d; p = M [pc;1] as ((m0 x + m1 y) + m2 z) + m3 without fused multiply-add; crop lo <= p < hi.
 *   points [C,cap,3]; source: the linear pixel.
 * bds_pseudo_lidar_from_points -- pto_ang_map_vertical (generate_lidar/generate_lidar_from_depth.py:42-92) and pto_ang_map /
 *   gen_sparse_points (generate_lidar/depth2lidar.py:41-90) for a cloud [N,4] (x, y, z, intensity; FINITE, 16-byte aligned): no
 *   unprojection and no matrix, the crop applied when crop = 1, the row is the key.  points [cap,4]: the winners' rows, copied;
 *   winner [H,W], counts [1], source [cap] or NULL.  N = 0 gives counts = 0.
 * Both: BDS_EINVAL before any launch for H, W or slice below 1, an unknown mode, a NULL or misaligned array that the call would read
 * or write, C above 65535, or C*Hi*Wi, N, C*H*W or 4*C*cap above 2^31 - 257.  C = 0: nothing to do. */
#define BDS_PSEUDO_LIDAR_BEAMS 12
#define BDS_PSEUDO_LIDAR_VERTICAL 0
#define BDS_PSEUDO_LIDAR_CLASSIC 1
int bds_pseudo_lidar_from_depth(int C, int Hi, int Wi, const float *depth, const float *cams, const double *beams, int H, int W,
                                int slice, int mode, int32_t *winner, float *points, int32_t *counts, int32_t *source,
                                bds_stream_t stream);
int bds_pseudo_lidar_from_points(int64_t N, const float *cloud, const double *beams, int crop, int H, int W, int slice, int mode,
                                 int32_t *winner, float *points, int32_t *counts, int32_t *source, bds_stream_t stream);

/* A view's input preparation: what CameraData.get_image (datasets/base/pixel_source.py:477-657) makes in front of every training step
 * and every evaluation render, and ScenePixelSource.prepare_novel_view_render_data (:1070-1132) for a novel trajectory.  Pointers +
 * stream, no allocation, no read-back, one launch each, no atomics: bit-identical run to run.  All math is float32, every operation
 * rounded on its own (no fused multiply-add); divisions and the square root are correctly rounded.
 * bds_view_fields -- every per-pixel field of B views (get_rays, pixel_source.py:38-75, and the fills and pixel_coords of :507-630).
 *   c2w [B,4,4] and intrinsics [n_intrinsics,3,3] (n_intrinsics = 1: one matrix for all views, or B), unscaled; the kernel forms
 *   fx = K[0][0] scale, fy = K[1][1] scale, cx = K[0][2] scale, cy = K[1][2] scale as ``intrinsics * downscale_factor`` does (:625).
 *   Per pixel (x = column, y = row): dx = ((x - cx) + 0.5) / fx, dy = ((y - cy) + 0.5) / fy; dir_i = (dx R[i][0] + dy R[i][1]) +
 *   R[i][2]; n = sqrt((d0 d0 + d1 d1) + d2 d2); viewdirs = dir / (n + 1e-8); origins = c2w[:3,3]; pixel_coords = (float(y) /
 *   float(H), float(x) / float(W)), row first.  normed_time [B] float32 and ids [B,3] int64 (image, frame, camera) ON THE DEVICE
 *   are the fills' values.  Outputs, each NULL to skip it, 16-byte aligned: origins, viewdirs [B,H,W,3], direction_norm [B,H,W,1],
 *   pixel_coords [B,H,W,2], normed_time_out [B,H,W] (needs normed_time), img_idx, frame_idx, cam_id [B,H,W] int64 (need ids),
 *   intrinsics_out [B,3,3]: intrinsics * scale with [2][2] = 1 (:625-626).  B = 0 or H W = 0: nothing to do.  BDS_EINVAL before the
 *   launch for a negative size, B above 65535, B H W above 2^31 - 257, a NULL c2w or intrinsics, n_intrinsics neither 1 nor B, a
 *   scale that is not positive and finite, a misaligned array or a missing fill source.
 * bds_image_resize_aa -- F.interpolate(mode="bicubic", antialias=True, scale_factor=factor) of an image [H,W,3] (:492-502, without
 *   its two permutes) into out [floor(H factor), floor(W factor), 3], contiguous.  Per axis: scale = (float)(1 / factor), support =
 *   2 scale; output i takes the taps [lo, lo + n), c = scale (i + 0.5), lo = max(0, int(c - support + 0.5)), n = min(in, int(c +
 *   support + 0.5)) - lo, with weights cubic((j + lo - c + 0.5) / scale), Keys' a = -0.5, divided by their sum; width first, then
 *   height.  1 / BDS_PIXELS_MAX_SCALE <= factor <= 1 (the reference never enlarges; a window of more than 4 * 512 + 3 taps per axis
 *   does not fit a workgroup's LDS): BDS_EINVAL otherwise.
 * bds_masks_resize_nearest -- F.interpolate(mode="nearest", scale_factor=factor) of n <= BDS_PIXELS_MAX_MASKS masks [H,W] float32
 *   (:520-579) into [floor(H factor), floor(W factor)] each, in one launch: source index min(int(floorf(dst * (float)(1 / factor))),
 *   in - 1) per axis, values copied.  in, out: HOST arrays of n device pointers.  BDS_EINVAL for n above the maximum, a factor
 *   outside (0, 1] or a NULL pointer. */
#define BDS_PIXELS_MAX_MASKS 5
#define BDS_PIXELS_MAX_SCALE 512
int bds_view_fields(int B, int H, int W, const float *c2w, const float *intrinsics, int n_intrinsics, float scale,
                    const float *normed_time, const int64_t *ids, float *origins, float *viewdirs, float *direction_norm,
                    float *pixel_coords, float *normed_time_out, int64_t *img_idx, int64_t *frame_idx, int64_t *cam_id,
                    float *intrinsics_out, bds_stream_t stream);
int bds_image_resize_aa(int H, int W, double factor, const float *in, float *out, bds_stream_t stream);
int bds_masks_resize_nearest(int n, int H, int W, double factor, const float *const *in, float *const *out, bds_stream_t stream);

/* The error-driven image sampler's maps (CameraData.update_image_error_maps, datasets/base/pixel_source.py:431-449, and the per-image
 * means of ScenePixelSource.update_image_error_maps :948-983) of B rendered views [h,w] in one call: pointers + stream, no allocation,
 * no read-back, two launches (the maps with one partial per workgroup, then the statistics), no atomics: bit-identical run to run.
 * pred, gt [B,h,w,3] float32, dyn [B,h,w] float32 or NULL (no dynamic opacity).  Per pixel (csrc/error_buffer_math.h):
 *   e = ((|g0 - c0| + |g1 - c1|) + |g2 - c2|) / 3, c = clamp(p, 0, 1) (render_images' clamp, models/video_utils.py:185-187; gt is not
 *   clamped), e * 5 where dyn > 0.1f, strictly; float32, every operation rounded on its own; a NaN in p or g gives a NaN e.
 * slots, img_ids [B] int64 ON THE DEVICE: view b's map goes to maps[slots[b]] (maps [F,h,w]) and its statistics to stats[img_ids[b]]
 * (stats [num_imgs,3]: mean, min, max of the view's e).  The mean is summed in double in a fixed order, divided by h w and rounded to
 * float32 once; min and max propagate a NaN.  The slots of one call must differ, and so must the ids.  Rows of maps and stats that no
 * view names keep their bits; a slot outside [0, F) or an id outside [0, num_imgs) drops that view's map or statistics (nothing is
 * written out of bounds).  Views whose bases are 16-byte aligned move 16 bytes per access, others 4: the results are the same bits.
 * ws: bds_error_maps_workspace_bytes(B, h, w) bytes, 16-byte aligned.  0 with nothing done for B = 0; for h w = 0 the named stats rows
 * become NaN (the mean of nothing) where stats and img_ids are given.  BDS_EINVAL before any launch: a negative extent, F or num_imgs,
 * B h w above 2^31 - 1 (the size query then answers 0), more than 2^24 - 1 workgroups (one per 1024 pixels of a view, at most 1024 per
 * view), a NULL pred / gt / slots / img_ids / maps / stats / ws, a misaligned pointer (4 bytes; slots, img_ids 8; ws 16), or a
 * workspace that is too small. */
size_t bds_error_maps_workspace_bytes(int B, int h, int w);
int bds_error_maps(int B, int h, int w, const float *pred, const float *gt, const float *dyn, const int64_t *slots,
                   const int64_t *img_ids, float *maps, int F, float *stats, int num_imgs, void *ws, size_t ws_bytes,
                   bds_stream_t stream);

/* One finished uint8 frame of an evaluation video (save_concatenated_videos, models/video_utils.py:703-768, and save_seperate_videos
 * :771-857, with the dataset layouts, to8b and depth_visualizer of utils/visualization.py:19-22, 41-341, 412-497): where the reference
 * colours, tiles, concatenates and quantises every timestep in numpy from host copies of the renders, one launch writes the canvas
 * [Hc,Wc,3] uint8 from the device tensors.  panels: a HOST array of n_panels rectangles of the canvas, read during the call (passed on
 * to the kernel by value: no upload, no allocation, nothing the stream outlives).  A panel shows rows [src_row0, src_row0 + dst_h) and
 * columns [0, dst_w) of its source [src_h,src_w] at (dst_y, dst_x); where panels overlap the LATER one wins, as the reference's
 * successive assignments do; a pixel in no panel is 0.  Every byte of the canvas is written: no memset precedes the call.  No
 * atomics, no read-back: bit-identical run to run.  Per pixel (csrc/video_math.h), by kind:
 *   BDS_VIDEO_RGB             src0 [src_h,src_w,3] float32: (uint8)(255.0f * clamp(x, 0, 1)) per channel, truncated (to8b); a NaN gives 0
 *   BDS_VIDEO_GRAY            src0 [src_h,src_w] float32, or bytes (bool, uint8) with BDS_VIDEO_SRC0_BYTES: the same, replicated to three
 *                             channels (the ``*mask*`` keys and gt_sky_masks, :735-740)
 *   BDS_VIDEO_DEPTH           src0 depth float32, src1 weight float32, bytes with BDS_VIDEO_SRC1_BYTES, or NULL (1): turbo's entry
 *                             min((int)(s * 256.0f), 255), s = clamp((-logf(d + 1e-6f) - min(lo, hi)) / |hi - lo|, 0, 1) * weight with
 *                             lo = -log(4 + 1e-6), hi = -log(120 + 1e-6) (depth_visualizer, :741-756); a NaN s is 0, a NaN product black
 *   BDS_VIDEO_OVER_GREEN      src0 rgb [.,.,3], src1 opacity [.,.] float32: to8b(clamp(rgb, 0, 1) * op + (0, 177, 64) / 255 * (1 - op))
 *                             (:201-227 behind the clamp of :185-187)
 *   BDS_VIDEO_LIDAR_ON_IMAGE  src0 pixels [.,.,3], src1 lidar depth map [.,.] float32: the depth's colour with weight 1 where it is
 *                             > 0, else to8b of the pixel (:265-271)
 * More than BDS_VIDEO_MAX_PANELS panels: one launch per band of rows that at most that many panels touch.
 * BDS_OK with nothing done for Hc Wc = 0.  BDS_EINVAL before any launch: a negative count or extent, Hc Wc 3 or a source's
 * src_h src_w 3 above 2^31 - 1, a NULL or misaligned (4 bytes) canvas, a NULL panels with n_panels > 0, and per panel an unknown kind or
 * flag, a NULL src0 (src1 where the kind needs it), a float32 source off a 4-byte boundary, a rectangle outside the canvas or source
 * rows or columns outside the source.  BDS_ECAPACITY: more than BDS_VIDEO_MAX_PANELS panels touch one row. */
#define BDS_VIDEO_MAX_PANELS 64
#define BDS_VIDEO_RGB 0
#define BDS_VIDEO_GRAY 1
#define BDS_VIDEO_DEPTH 2
#define BDS_VIDEO_OVER_GREEN 3
#define BDS_VIDEO_LIDAR_ON_IMAGE 4
#define BDS_VIDEO_SRC0_BYTES 1
#define BDS_VIDEO_SRC1_BYTES 2
typedef struct bds_video_panel {
  const void *src0, *src1;
  int32_t kind, flags;
  int32_t src_h, src_w, src_row0;
  int32_t dst_y, dst_x, dst_h, dst_w;
  int32_t reserved; /* 0 */
} bds_video_panel;
int bds_video_frame(int n_panels, const bds_video_panel *panels, int Hc, int Wc, uint8_t *canvas, bds_stream_t stream);

/* Lens undistortion of F frames [H,W,C] of bytes (C = 1 or 3) in one call: what cv2.undistort does frame by frame on the host in
 * CameraData.load_images, load_egocar_mask, load_dynamic_masks and load_sky_masks.  Pointers + stream, no allocation, no read-back,
 * one launch (one per 65535 frames), no atomics: bit-identical run to run.  OpenCV is not installed where this is built: the
 * algorithm (csrc/undistort_math.h) restates OpenCV 4.x's published one, PARITY UNPINNED.
 *   cams [F,18] doubles ON THE DEVICE, 8-byte aligned, per frame: fx, fy, u0, v0 of the camera matrix | k1, k2, p1, p2, k3 | the nine
 *   entries of inverse(new camera matrix), row-major, formed by the caller in double (the new matrix is the camera matrix itself in
 *   cv2.undistort's default form).
 *   Per output pixel (row i, column j), in double, every operation rounded on its own: (_x, _y, _w) = ir (j, i, 1); x = _x / _w,
 *   y = _y / _w; r2 = x x + y y; kr = 1 + ((k3 r2 + k2) r2 + k1) r2; xd = x kr + p1 (2 x y) + p2 (r2 + 2 x x); yd = y kr +
 *   p1 (r2 + 2 y y) + p2 (2 x y); u = fx xd + u0, v = fy yd + v0.  iu = rint(32 u), iv = rint(32 v), half to even, saturated to
 *   int32; sx = iu >> 5, ax = iu & 31, sy = iv >> 5, ay = iv & 31 (floor and rest); the four 15-bit weights (32 - ay)(32 - ax) 32,
 *   (32 - ay) ax 32, ay (32 - ax) 32, ay ax 32 of the taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1); per channel
 *   (sum of tap x weight + 16384) >> 15 in integers.  The border is a constant 0: a tap outside the image contributes 0, and the
 *   pixel is 0 when sx >= W, sx + 1 < 0, sy >= H or sy + 1 < 0.  Deviations from OpenCV: the image is one stripe (OpenCV shifts v0 per
 *   stripe of rows), and a coordinate beyond +-32767 px counts as outside (OpenCV's 16-bit map wraps there).
 *   out_kind: BDS_UNDISTORT_UINT8 -- out [F,H,W,C] bytes; BDS_UNDISTORT_UNIT -- float32, value / 255 (the image stack's ``/ 255``);
 *   BDS_UNDISTORT_MASK -- float32, value > 0 ? 1 : 0 (the masks' ``> 0`` then ``.float()``).  Every element of out is written.
 * All indexing is 64-bit.  BDS_EINVAL before any launch: a NULL pointer, F, H or W below 1, H or W above 32767, C other than 1 or 3,
 * an unknown out_kind, cams off an 8-byte or a float32 out off a 4-byte boundary. */
#define BDS_UNDISTORT_UINT8 0
#define BDS_UNDISTORT_UNIT 1
#define BDS_UNDISTORT_MASK 2
/* datasets/base/pixel_source.py:249-256,273-278,296-303,319-326,342-349,366-373 (cv2.undistort) */
int bds_undistort(int F, int H, int W, int C, const uint8_t *src /*[F,H,W,C]*/, const double *cams /*[F,18]*/,
                  int out_kind, void *out, bds_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BDS_H */
