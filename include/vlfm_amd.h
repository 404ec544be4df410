/*
 * vlfm_amd.h -- C ABI of libvlfm_amd.so: the MI355X (gfx950) implementation of VLFM's per-step
 * perception + mapping hot path.
 *
 * The reference has no FFI for this path: its boundary is the Python class API of
 * vlfm.mapping.{ValueMap,ObstacleMap} and vlfm.vlm.*Client.  The functions below are what a ctypes
 * binding inside those classes calls (INTEGRATION.md shows the stub); each one cites the reference
 * lines it replaces.  Conventions:
 *   - extern "C", plain pointers + sizes, no ownership transfer, no hidden allocation in step calls
 *   - pointers prefixed d_ are DEVICE pointers (HBM of the current HIP device), h_ are HOST pointers
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream)
 *   - return 0 on success, <0 = vlfm_status (mapped to the reference's Python exceptions by the host layer)
 *   - all kernels are batched over `n` environment slots; maps are [n_envs][S][S] resident in HBM
 */
#ifndef VLFM_AMD_H
#define VLFM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    VLFM_OK = 0,
    VLFM_ERR_INVALID = -1,       /* bad argument (null pointer, non-positive size, unsupported shape) */
    VLFM_ERR_OUTSIDE_MAP = -2,   /* camera / waypoint cell outside the map: AssertionError "Pixel location is
                                    outside the image." (vlfm/utils/img_utils.py:43, :235-237) */
    VLFM_ERR_INDEX = -3,         /* obstacle scatter hit a cell >= S: IndexError (vlfm/mapping/obstacle_map.py:101,
                                    caught by vlfm/policy/base_objectnav_policy.py:157-162) */
    VLFM_ERR_HIP = -4,           /* a HIP runtime call failed (see vlfm_last_error) */
    VLFM_ERR_CAPACITY = -5       /* a caller-provided scratch/output capacity was too small */
} vlfm_status;

/* fusion modes of ValueMap._fuse_new_data (vlfm/mapping/value_map.py:377-429) */
enum { VLFM_FUSE_DEFAULT = 0, VLFM_FUSE_REPLACE = 1, VLFM_FUSE_EQUAL_WEIGHTING = 2 };

const char* vlfm_last_error(void);
int vlfm_abi_version(void);

/* Optional per-kernel timing: on = 1 brackets every kernel launch of this library with hipEvents on its launch stream,
 * on = n > 1 every n-th launch of each kernel (sampling: a timed dispatch costs host time and keeps the runtime's
 * completion thread awake), 0 switches it off.  kernel_name is the device function's name (e.g. "depth_ingest_kernel"). */
int vlfm_profile_enable(int on);
int vlfm_profile_read(const char* kernel_name, double* mean_ms, int* launches);

/* How the CURRENT device's host waits (hipStreamSynchronize / hipEventSynchronize, also PyTorch's) behave: blocking != 0
 * selects hipDeviceScheduleBlockingSync (the waiting thread sleeps on the completion interrupt), 0 restores the
 * runtime's default (hipDeviceScheduleAuto: a busy wait that holds one host core for as long as the GPU runs).  With one
 * rank per GPU and ~100 ms of queued perception work per step the busy wait is what fills the node's CPU quota; the
 * reference has no counterpart (its per-step waits are blocking socket reads, vlfm/vlm/server_wrapper.py:78-109). */
int vlfm_host_wait_mode(int blocking);

/* ---------------------------------------------------------------------------------------------
 * Per-observation pose parameters of one value-map update (64 bytes, uploaded to HBM by the caller).
 * Filled on the host by vlfm_value_map_pose_params(); consumed by vlfm_value_map_update_fused_batched().
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    double inv_affine[6]; /* dst->src 2x3 matrix cv::warpAffine derives from getRotationMatrix2D
                             (vlfm/utils/img_utils.py:23-26) */
    int32_t row0, col0;   /* map cell of the template's top-left corner (may be negative; clipped on device)
                             = camera cell - T/2, camera cell by truncation (vlfm/mapping/value_map.py:309-313) */
    int32_t env;          /* environment slot the observation belongs to */
    int32_t reserved;
} vlfm_vm_pose;

/* Host: restates ValueMap._localize_new_data's scalar prologue (value_map.py:297-313) + rotate_image's matrix
 * (img_utils.py:23-25) for n observations.  h_tf: [n][16] row-major camera->episodic transforms (f64).
 * h_yaw: [n] yaw angles if the caller already evaluated extract_yaw (geometry_utils.py:145-159) -- a Python host
 * passes numpy.arctan2's result so that the angle is the reference's to the last bit -- or NULL (libm atan2).
 * h_env: [n] env slot per observation (NULL = 0..n-1).  Returns VLFM_ERR_OUTSIDE_MAP if a camera cell falls
 * outside [0,S) (place_img_in_img's assertion, img_utils.py:43); *bad_index then holds the observation. */
int vlfm_value_map_pose_params(const double* h_tf, const double* h_yaw, const int32_t* h_env, int n, int map_size,
                               int pixels_per_meter, int template_size, vlfm_vm_pose* h_out, int* bad_index);

/* Host: the unmasked confidence table of ValueMap._get_confidence_mask (value_map.py:337-351) for a T x T
 * template, T = 2*int(max_depth*ppm)+1, plus the 16.16 fixed-point sector polygon cv2.ellipse rasterises for
 * ValueMap._get_blank_cone_mask (value_map.py:321-335).  h_conf: [T*T] f32.  h_poly_xy: [2*cap] int64.
 * Returns T (>0) or a negative status. */
int vlfm_cone_template_host(double fov, double max_depth, int pixels_per_meter, double min_confidence,
                            float* h_conf, int conf_capacity, int64_t* h_poly_xy, int poly_capacity,
                            int* n_poly);

/* Host: tan(linspace(-fov/2, fov/2, W)) in f64 (value_map.py:237,242). */
int vlfm_tan_table_host(double fov, int width, double* h_out);

/* Device: d_template[T*T] = inside(sector polygon) ? d_conf[T*T] : 0, and d_template_bits [T][ceil(T/32)] = the bit
 * plane (d_template > 0).  One workgroup; once per (fov, max_depth), like the reference's cache (value_map.py:37). */
int vlfm_cone_template_build(const float* d_conf, const int64_t* d_poly_xy, int n_poly, int template_size,
                             float* d_template, uint32_t* d_template_bits, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth ingest: ONE pass over each depth image feeding both maps.
 *   (a) column max  -> d_colmax[n][W]      (np.max(depth, axis=0), value_map.py:234)
 *   (b) obstacle scatter -> d_obstacle[env][S][stride] bit-packed (unproject, transform, height band, rint cell, set bit;
 *       obstacle_map.py:92-101 + geometry_utils.py:205-236 + base_map.py:44-46)          [optional]
 * d_depth: [n][H][W] f32 in [0,1].
 * d_colmax_keys [n][W] u32: column maxima as order-preserving keys (0 = -inf).  The buffer must be zero when the call
 * is made: allocate it zeroed once; vlfm_value_map_update_fused_batched consumes the keys and writes the zeros back, so a
 * steady ingest -> update cadence needs no memset.  d_status [n][2] is sticky: the kernel only ever sets flags in it;
 * the caller zeroes it after reading.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    double tf[12];        /* first three rows of the camera->episodic 4x4 (row-major) */
    float depth_scale;    /* f32(max_depth - min_depth) */
    float depth_offset;   /* f32(min_depth) */
    float depth_max;      /* f32(max_depth) */
    float reserved0;
    double fx, fy;
    double min_height, max_height;
    int32_t env;          /* obstacle-map slot */
    int32_t scatter;      /* bit 0: scatter obstacles (0 = column max only, update_obstacles=False);
                             bit 1: every zero depth texel is a filled hole (hole_area_thresh == -1, obstacle_map.py:87-89);
                             bit 2: zero texels are left to vlfm_depth_scatter_holes_batched (their fate depends on
                                    fill_small_holes, which needs the whole image first) */
} vlfm_ingest_params;     /* 152 bytes */

/* Undo journal of the speculative single depth pass (fill_small_holes mode).  The pass places every NON-zero texel before
 * fill_small_holes has run; a valid texel that lies INSIDE a filled hole contour (an "island": the reference's
 * drawContours(.., -1) covers it, it becomes 1.0 and is dropped, img_utils.py:385-388) must not count.  The pass
 * therefore records the cell id (row * S + col) of every obstacle bit it is the FIRST to set; for island frames
 * vlfm_fill_small_holes_batched clears exactly those bits and vlfm_depth_scatter_holes_batched re-places the valid
 * texels outside the filled area.  d_count must be zero on entry (allocate zeroed; vlfm_fill_small_holes_batched
 * resets it -- a caller whose vlfm_depth_ingest_batched was NOT followed by vlfm_fill_small_holes_batched, e.g. after an
 * error in between, zeroes d_count itself before the next ingest, or a later island frame would undo that step's bits).
 * In this mode a texel that falls off the map is only NOTED by the ingest (status word 1, bit 1): whether the reference
 * would have scattered it is decided by fill_small_holes, which promotes the note to VLFM_ERR_INDEX in status word 0
 * unless the frame has islands (their surviving texels are placed, and judged, again by the hole scatter).
 * Observations of one call must belong to distinct environment slots when a journal is used -- or go through the *_rig_batched
 * forms of the two follow-up calls below. */
typedef struct {
    uint32_t* d_cells;    /* [n][capacity] */
    int32_t* d_count;     /* [n] */
    int32_t capacity;     /* entries per observation; (2*ceil(reach*ppm)+3)^2 is always enough */
    int32_t reserved;
} vlfm_scatter_journal;   /* 24 bytes, HOST struct holding device pointers */

int vlfm_depth_ingest_batched(const float* d_depth, int n, int height, int width,
                              const vlfm_ingest_params* d_params,
                              uint32_t* d_colmax_keys /* [n][W] or NULL */,
                              uint32_t* d_obstacle /* [n_envs][S][ceil(S/32)] bit-packed or NULL */, int map_size, int pixels_per_meter,
                              int32_t* d_status /* [n][2] sticky: [0] VLFM_ERR_INDEX if a point fell off the map,
                                                   [1] bit 0: the image holds a zero (invalid) depth texel; bit 1: the
                                                   speculative pass (journal mode) hit a cell off the map */,
                              uint32_t* d_hole_bits /* OUT [n][H][ceil(W/32)] bit plane of (depth == 0), or NULL */,
                              const uint32_t* d_filled_bits /* IN  [n][H][ceil(W/32)] texels fill_small_holes set to
                                                               1.0 (vlfm_fill_small_holes_batched), or NULL */,
                              const vlfm_scatter_journal* journal /* host pointer or NULL (see above) */,
                              void* stream);

/* Diagnostic: the depth scatter divides by the focal lengths with a hoisted reciprocal and one FMA correction step (same bits
 * as the IEEE division, a quarter of its instructions).  Counts into d_mismatches[0] (caller zeroes it) the numerators for
 * which that quotient differs from __ddiv_rn(numerator, divisor): must stay 0. */
int vlfm_selftest_div_exact(const double* d_numerators, int n, double divisor, int32_t* d_mismatches, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fill_small_holes (vlfm/utils/img_utils.py:361-390) for n depth images, on the bit plane (depth == 0) produced by
 * vlfm_depth_ingest_batched: cv2.findContours(RETR_TREE, CHAIN_APPROX_SIMPLE) = every outer AND hole border, in OpenCV's
 * order; each border whose cv2.contourArea is < area_thresh is drawn filled (cv2.drawContours(.., 1, -1)) into
 * d_filled_bits.  One workgroup per image; images whose status word [1] is 0 (no zero texel) cost one early exit and
 * get an all-zero d_filled_bits only if they had holes before (see d_dirty).
 *   d_status   [n][2] the ingest status (word 1: bit 0 = image has zeros, bit 1 = speculative off-map hit; consumed here)
 *   d_scratch  vlfm_hole_scratch_bytes(n, H, W, cap_pts, cap_contours) bytes
 *   d_counts   [n][4] int32: (contours traced, contours filled, overflow flags: bit 0 contour scratch, bit 1 journal,
 *              bit 0 image had zero texels | bit 1 island frame = valid texels inside a filled contour)
 *   d_params / d_obstacle / map_size / journal: only with a journal (else NULL / NULL / 0 / NULL): the env slot of each
 *              observation, the obstacle planes and the undo journal of the speculative pass
 * Single depth pass (what ObstacleMapBatch does): vlfm_depth_ingest_batched with scatter bits 0|2 and a journal places
 * every NON-zero texel and writes d_hole_bits; this call decides which zeros become 1.0 and, for island frames, takes the
 * speculative pass's new bits back; vlfm_depth_scatter_holes_batched then places the zeros that survived (depth 0 ->
 * z = min_depth) from the two bit planes and -- island frames only, which is the one case that reads d_depth again --
 * the valid texels outside the filled area.
 * (Alternative without a journal: vlfm_depth_ingest_batched with scatter bit 0 clear, this call, then a second
 * vlfm_depth_ingest_batched with d_filled_bits and d_colmax_keys = NULL.)
 * ------------------------------------------------------------------------------------------- */
size_t vlfm_hole_scratch_bytes(int n, int height, int width, int cap_pts, int cap_contours);
int vlfm_fill_small_holes_batched(const uint32_t* d_hole_bits, const int32_t* d_status, int n, int height, int width,
                                  double area_thresh, void* d_scratch, size_t scratch_bytes, int cap_pts,
                                  int cap_contours, uint32_t* d_filled_bits, int32_t* d_counts,
                                  const vlfm_ingest_params* d_params, uint32_t* d_obstacle, int map_size,
                                  const vlfm_scatter_journal* journal, void* stream);
int vlfm_depth_scatter_holes_batched(const vlfm_ingest_params* d_params, int n, int height, int width,
                                     const uint32_t* d_hole_bits, const uint32_t* d_filled_bits,
                                     const int32_t* d_hole_counts /* d_counts of vlfm_fill_small_holes_batched */,
                                     uint32_t* d_obstacle, int map_size, int pixels_per_meter, int32_t* d_status,
                                     const float* d_depth /* [n][H][W]: read for island frames only; NULL = never */,
                                     void* stream);

/* Camera rig: the same two calls when SEVERAL observations of the launch may belong to one slot (the robot's body cameras,
 * reality_policies.py:113-138: the obstacle scatter is a pure OR, so the cameras of a step commute in the reference).  The
 * speculative pass journals a bit for the ONE observation that set it first; if that observation turns out to be an island
 * frame the undo would remove a bit a sibling frame legitimately placed (sequentially, the island frame would have been
 * undone before the sibling ran).  d_slot_undone [n_envs] int32 (zeroed by the fill call) is set for every slot that had a
 * frame undone; the scatter call then places the valid texels outside the filled area of EVERY frame of such a slot again,
 * from d_depth (required).  Frames of slots without an island frame are read once, as in the single-camera form. */
int vlfm_fill_small_holes_rig_batched(const uint32_t* d_hole_bits, const int32_t* d_status, int n, int height, int width,
                                      double area_thresh, void* d_scratch, size_t scratch_bytes, int cap_pts,
                                      int cap_contours, uint32_t* d_filled_bits, int32_t* d_counts,
                                      const vlfm_ingest_params* d_params, uint32_t* d_obstacle, int map_size,
                                      const vlfm_scatter_journal* journal, int32_t* d_slot_undone, int n_envs, void* stream);
int vlfm_depth_scatter_holes_rig_batched(const vlfm_ingest_params* d_params, int n, int height, int width,
                                         const uint32_t* d_hole_bits, const uint32_t* d_filled_bits,
                                         const int32_t* d_hole_counts, uint32_t* d_obstacle, int map_size,
                                         int pixels_per_meter, int32_t* d_status, const float* d_depth,
                                         const int32_t* d_slot_undone, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ValueMap.update_map for n observations (value_map.py:100-128 = :221-260 + :288-319 + :357-429) in ONE launch: every workgroup
 * rasterises the depth-profile polygon of its observation into LDS itself, so no visibility plane goes through HBM and no scratch
 * is needed.
 *   d_colmax_keys [n][W]     column-max keys from depth ingest (consumed: reset to 0 by this call)
 *   d_tan      [W]           f64 tan table (vlfm_tan_table_host)
 *   d_template [T*T]         f32 masked confidence template;  d_template_bits [T][ceil(T/32)] its (> 0) bit plane
 *   d_pose     [n]           vlfm_vm_pose
 *   d_values   [n][C]        f64 values (BLIP-2 cosines)
 *   d_conf     [n_envs][S][S]      f32 confidence maps   (BaseMap._map)
 *   d_value    [n_envs][S][S][C]   f64 value maps        (ValueMap._value_map).  f64 because the reference's array IS f64
 *              after the first weighted fuse (`values` is an f64 ndarray; value_map.py:423 re-binds `_value_map` to the
 *              f64 result) and stays f64; in the modes where it stays f32 (use_max_confidence :406, fusion "replace"
 *              :381-384) the stored doubles are f32-representable.  Either way the array equals the reference's bit for bit.
 *   d_explored_bits [n_envs][S][ceil(S/32)] bit-packed ObstacleMap.explored_area when the value map was built with
 *              obstacle_map=... (value_map.py:369-375), or NULL = Habitat default (windowed update, exact).
 *   d_written_bits [n_envs][S][ceil(S/32)] bit plane, zero at reset, owned by the caller and maintained by this call:
 *              bit = the cell has received a confidence.  Required with d_explored_bits (NULL otherwise): the full-map
 *              half of _fuse_new_data (value_map.py:369-375: conf = value = 0 wherever explored == 0) then clears exactly
 *              the cells in (written & ~explored) -- every other cell is zero already.  Observations of one call must
 *              belong to distinct environment slots.
 *   d_counters [n] int32, zero on entry and zero again on exit (hand-over of the column-max key buffer).
 *   d_conf_quadrant [(T/2+1)^2] f32: rows/cols >= T/2 of the UNMASKED confidence table of vlfm_cone_template_host (the
 *              table depends on |row - T/2| and |col - T/2| only, value_map.py:343-351).  Staged in LDS so that the rotated
 *              template taps are LDS reads (required).
 * (Rounds 1-5 also exported the three-launch form this replaced -- mask_unexplored + visible_mask + fuse; removed in round 6.)
 * ------------------------------------------------------------------------------------------- */
int vlfm_value_map_update_fused_batched(uint32_t* d_colmax_keys, int width, const double* d_tan,
                                        const float* d_template, const uint32_t* d_template_bits, int template_size,
                                        const vlfm_vm_pose* d_pose, const double* d_values, int n,
                                        float* d_conf, double* d_value, int map_size, int channels, int pixels_per_meter,
                                        double min_depth, double max_depth, int use_max_confidence, int fusion_type,
                                        const uint32_t* d_explored_bits, uint32_t* d_written_bits, int32_t* d_counters,
                                        const float* d_conf_quadrant, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Camera rig: ValueMap.update_map for n observations of which SEVERAL may belong to one environment slot, in one launch.
 * The observations of a slot are applied in the order given -- exactly the reference's sequential loop over its cameras
 * (itm_policy.py:191-211; reality_policies.py:113-141), whose weighted fuse does not commute -- and different slots run
 * concurrently.  The result equals n single-observation calls of vlfm_value_map_update_fused_batched bit for bit.
 * Each observation brings its own optics (the reference passes min_depth / max_depth / fov per camera):
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    const float* d_template;         /* [T*T] masked confidence template of (fov, max_depth) (not read by the kernel today) */
    const uint32_t* d_template_bits; /* [T][ceil(T/32)] its (> 0) bit plane */
    const float* d_conf_quadrant;    /* [(T/2+1)^2] quadrant of the unmasked table */
    const double* d_tan;             /* [W] tan table of (fov, W) */
    float depth_scale;               /* f32(max_depth - min_depth) */
    float depth_offset;              /* f32(min_depth) */
    int32_t template_size;           /* T = 2*int(max_depth*ppm)+1 */
    int32_t reserved;
} vlfm_vm_optics;                    /* 48 bytes */

/*   d_pose / d_optics [n]  GROUPED BY SLOT: the observations of a slot are consecutive and in application order;
 *                          d_pose[i].reserved = the observation's row in d_colmax_keys, d_values and d_counters (its position
 *                          in the caller's own list, so that keys written by a depth ingest need no reordering)
 *   d_slots [n_slots][2]   int32 (first, count) into d_pose / d_optics, one entry per slot present in the call
 *   max_template_size      the largest template_size among d_optics (sizes the workgroup's LDS).  d_optics is device data:
 *                          the call cannot check it, a record with a larger template_size would overrun the LDS arrays
 *   all observations share the image width (mixed widths: separate calls); the other arguments are those of
 *   vlfm_value_map_update_fused_batched.  With d_explored_bits the (written & ~explored) clear runs once per slot before
 *   its first camera (the plane does not change within the call, and fused cells are explored ones), the mask applies to
 *   every camera.
 * Scheduling: grid (G, n_slots); 8-row tile b of the MAP belongs to workgroup b mod G of its slot for the whole launch, so a
 * map cell has one owner and no workgroup ever waits for another one. */
int vlfm_value_map_update_rig_batched(uint32_t* d_colmax_keys, int width, const vlfm_vm_pose* d_pose,
                                      const vlfm_vm_optics* d_optics, const int32_t* d_slots, int n_slots, int n,
                                      int max_template_size, const double* d_values, float* d_conf, double* d_value,
                                      int map_size, int channels, int pixels_per_meter, int use_max_confidence,
                                      int fusion_type, const uint32_t* d_explored_bits, uint32_t* d_written_bits,
                                      int32_t* d_counters, void* stream);

/* ValueMap.sort_waypoints scoring (value_map.py:146-187 + img_utils.py:213-266): per waypoint and channel the
 * median of the positive cells inside the radius disc, -1 if none.
 *   d_cells  [m][3] int32: (env, row, col) of each waypoint (host computes them by truncation, value_map.py:164-167)
 *   d_disc   [(2r+1)] int32 half-widths per disc row (cv2.circle raster, produced by vlfm_disc_rows_host)
 *   value_is_f32  non-zero when the reference's `_value_map` is still an f32 array in this map's mode (use_max_confidence
 *            or fusion "replace", or no update yet): np.median then averages the two middle elements of an even count in
 *            f32; zero = f64 arithmetic (the default weighted mode)
 *   d_out    [m][C] f64 medians (np.median's result in the array's dtype, widened), -1 where the disc holds no positive cell
 */
int vlfm_disc_rows_host(int radius, int32_t* h_halfwidth /* [2r+1] */);
int vlfm_value_map_sort_waypoints_batched(const double* d_value, int map_size, int channels,
                                          const int32_t* d_cells, int m, int radius, const int32_t* d_disc,
                                          int value_is_f32, double* d_out, void* stream);


/* ---------------------------------------------------------------------------------------------
 * VLM-side kernels (vlfm/vlm/blip2itm.py:37-54; LAVIS eval transform + ITC head [ext])
 * ------------------------------------------------------------------------------------------- */

/* Host: Pillow's precompute_coeffs + normalize_coeffs_8bpc (bicubic, a=-0.5, antialiased) for one axis.
 * h_bounds [out_size][2] = (first tap, tap count); h_kk [out_size][ksize] 22-bit fixed-point taps. */
int vlfm_resample_coeffs_host(int in_size, int out_size, int32_t* h_bounds, int32_t* h_kk, int kk_capacity,
                              int* ksize_out);

/* Same for Pillow's BICUBIC (filter 0) or BILINEAR (filter 1) kernels. */
int vlfm_resample_coeffs_filter_host(int in_size, int out_size, int filter, int32_t* h_bounds, int32_t* h_kk,
                                     int kk_capacity, int* ksize_out);

/* Device: MobileSAM.segment_bbox preprocessing (vlfm/vlm/sam.py:54 -> SamPredictor.set_image [ext]): PIL BILINEAR resize
 * to (out_h, out_w) (longest side 1024), (x - mean) / std on the 0..255 scale, zero padding to pad x pad:
 * d_rgb [n][H][W][3] u8 -> d_out [n][3][pad][pad] f32.  d_tmp: [n][H][out_w][3] u8 scratch. */
int vlfm_preprocess_sam_batched(const uint8_t* d_rgb, int n, int height, int width, int out_h, int out_w,
                                const int32_t* d_hbounds, const int32_t* d_hk, int hksize,
                                const int32_t* d_vbounds, const int32_t* d_vk, int vksize,
                                const float* h_mean3, const float* h_std3, int pad_size, uint8_t* d_tmp, float* d_out,
                                void* stream);

/* Device: d_rgb [n][H][W][3] u8 -> d_out (out_dtype 0=f32, 1=f16, 2=bf16):
 * PIL.Image.resize((out,out), BICUBIC) (two 8-bit passes, d_tmp [n][H][out][3] u8 scratch) -> /255 -> (x-mean)/std.
 * patch_size == 0: d_out is [n][3][out][out] (ToTensor layout).  patch_size == P > 0 (P divides out): d_out is
 * [n][(out/P)^2][3*P*P], the im2col rows of a stride-P patch-embedding convolution (same values, GEMM-ready). */
int vlfm_preprocess_rgb_batched(const uint8_t* d_rgb, int n, int height, int width, int out_size,
                                const int32_t* d_hbounds, const int32_t* d_hk, int hksize,
                                const int32_t* d_vbounds, const int32_t* d_vk, int vksize,
                                const float* h_mean3, const float* h_std3, uint8_t* d_tmp, void* d_out,
                                int out_dtype, int patch_size, void* stream);

/* Device: ITC head epilogue.  d_proj [B][NQ][P] f32 = vision_proj(Q-Former query outputs) (the 768->256 GEMM itself is
 * a plain library GEMM), d_text [B][P] L2-normalised text features -> d_out [B] = max_q <normalize(proj_q), text>.
 * One wavefront per (image, query): L2 norm + dot by lane-strided loads and a 64-lane shuffle reduction, then the
 * max over queries.  NQ <= 64. */
int vlfm_itc_head_batched(const float* d_proj, int batch, int n_query, int proj_dim,
                          const float* d_text, float* d_out, void* stream);

/* Device: the ITC head of ONE image against T prompts.  d_proj [B][NQ][P] f32 as above, d_text_table [U][P] the unique
 * L2-normalised text features, d_text_index [B][T] int32 rows of that table -> d_out [B][T],
 * out[b][t] = max_q <proj[b][q], table[index[b][t]]> / max(|proj[b][q]|, 1e-12).  Every query row is read once: its norm
 * and the T dot products come from one pass.  For each (b, t) the bits are those of vlfm_itc_head_batched on image b
 * and that text row (same element order per lane, same shuffle tree).  NQ <= 64, U >= 1,
 * 1 <= T <= VLFM_ITC_MAX_PROMPTS (one accumulator per prompt in registers, one wavefront of the 512-thread block per
 * prompt for the max over queries).  An index outside [0, U) is never followed: that element of d_out is NaN (callers
 * validate indices when they build the index array). */
#define VLFM_ITC_MAX_PROMPTS 8
int vlfm_itc_head_multi(const float* d_proj, int batch, int n_query, int proj_dim, const float* d_text_table, int n_text,
                        const int32_t* d_text_index, int n_prompts, float* d_out, void* stream);

/* y = LayerNorm(x + c) * gamma + beta over the last dimension of f16 rows [rows][dim] (f32 statistics); c = f32 [dim]
 * per-channel constant or NULL.  Used by the ViT-g blocks of BLIP-2 (blip2itm.py): the projection / fc2 GEMMs accumulate
 * straight into the residual stream and their bias vectors, summed per layer on the host once, enter through c -- the
 * two residual-add kernels per block disappear.  dim % 8 == 0, dim <= 2048; y may alias x. */
int vlfm_layernorm_bias_f16(const void* d_x, const float* d_channel_bias, const void* d_gamma, const void* d_beta,
                            void* d_y, int rows, int dim, float eps, void* stream);

/* Self-attention of the ViT-g blocks: d_qkv [batch][tokens][3][heads][head_dim] f16 (the qkv GEMM's output as it is),
 * d_out [batch][tokens][heads][head_dim] f16 = softmax(q k^T * scale) v per (image, head), ready for the projection
 * GEMM.  Specialised for tokens == 257 and head_dim == 88 (ViT-g's native head width: the qkv and projection GEMMs keep
 * their original sizes); anything else returns VLFM_ERR_INVALID and the caller uses the library attention.  A persistent
 * kernel: one workgroup per CU walks its (image, head) items with K / V / Q arriving by LDS-DMA under the previous
 * item's MFMAs (150 KB of LDS), v_mfma_f32_32x32x16_f16, f32 softmax, the CLS query on the VALU. */
int vlfm_vit_attention_f16(const void* d_qkv, void* d_out, int batch, int tokens, int heads, int head_dim, float scale,
                           void* stream);

/* C[M][N] = epilogue(X[M][K] . W[N][K]^T + bias[N]): f16 operands and result, f32 accumulation on the matrix cores
 * (hand-written MFMA kernels, csrc/gemm_f16.hip: 256 x 256 x 64 tiles, LDS-DMA staging, 8-phase schedule).  epilogue 0 = bias
 * only, 1 = bias + EXACT (erf) GELU on the f32 accumulator -- the fc1 + GELU of the ViT-g MLP inside the forward of
 * blip2itm.py:52 in one pass (hipBLASLt's fused GELU is the tanh approximation) --, 2 (ABI 6) = accumulate, the residual-stream
 * GEMMs (projection, fc2): C = f16(f16(X . W^T + bias) + C) -- product and bias are rounded to f16, then added to the stream in
 * f32 and rounded once more, as `c + linear(x, w, bias)` in f16 does.  K % 64 == 0, N % 8 == 0, each operand below 4 GB; d_bias
 * may be NULL.  d_x, d_w, d_c and a non-NULL d_bias must be 16-byte aligned (VLFM_ERR_INVALID otherwise). */
int vlfm_gemm_f16_nt(const void* d_x, const void* d_w, const void* d_bias, void* d_c, int m, int n, int k, int epilogue,
                     void* stream);

/* (ABI 13) The two-piece split-precision projection in ONE pass of the same kernel: out = X[M][K] . (W1 + 2^-11 W2)[N_out][K]^T + bias,
 * f16 operands, f32 bias, f32 result, every output element fl(acc1 + fl(bias + 2^-11 acc2)) -- the arithmetic of the two f32-output
 * library GEMMs it replaces, smallest term first -- written once.  d_w_pair is [2 N_out][K] f16: for every block of 64 output
 * channels its 64 rows of W1, then its 64 rows of W2.  The result is BLOCK-MAJOR: d_out[block][m][64] f32 (block = channel / 64), so
 * the 64 channels of one head over consecutive rows are contiguous.  K % 64 == 0, N_out % 64 == 0; d_bias_f32 may be NULL.  Every
 * pointer must be 16-byte aligned (VLFM_ERR_INVALID otherwise). */
int vlfm_gemm_f16_pair_f32_nt(const void* d_x, const void* d_w_pair, const void* d_bias_f32, void* d_out, int m, int n_out, int k,
                              void* stream);

/* (ABI 13) The Q-Former's cross-attention in f32 (csrc/qformer_attention.hip): d_out[b][q][h * 64 ..] = softmax_t(scale * <q, K_t>) V_t
 * for d_q / d_out [batch][queries][heads * 64] f32 and K / V read from the block-major tensor of vlfm_gemm_f16_pair_f32_nt
 * ([blocks][m_total][64] f32): image b is rows [b * tokens, (b + 1) * tokens), head h of K is block k_block0 + h, of V block
 * v_block0 + h.  Head width 64; 1 <= queries <= 32, 1 <= tokens <= 257, batch * tokens <= m_total; anything else returns
 * VLFM_ERR_INVALID and the caller uses the library attention.  Rows of d_out beyond `batch` are not written. */
int vlfm_qformer_cross_attention_f32(const void* d_q, const void* d_kv_blocks, void* d_out, int batch, int tokens, int queries,
                                     int heads, int k_block0, int v_block0, int m_total, float scale, void* stream);

/* Diagnostic, host only (no GPU needed): the order in which vlfm_gemm_f16_nt's 8-phase kernels walk the 256 x 256 tiles of an
 * m x n result -- list position i -> (m-tile, n-tile) in out[2 i], out[2 i + 1]; position i runs on XCD i % 8, the persistent kernel's
 * workgroup w takes positions w, w + grid, ...  Returns the number of tiles (negative: error).  group_m <= 0: the default. */
int vlfm_gemm_f16_tile_order(int m, int n, int group_m, int* out, int capacity_pairs);
/* ... and the persistent kernel's work items for `grid` workgroups: item i -> (list position of its tile, n-half 0 / 1 or -1 = the whole
 * tile) in out[2 i], out[2 i + 1]; the tiles of a ragged last round are split into their two n-halves when that round is at most half
 * full.  Returns the number of items. */
int vlfm_gemm_f16_work_items(int m, int n, int grid, int* out, int capacity_pairs);

/* C[M][N] = act(X[M][K] . W[N][K]^T + bias[N]) + residual[M][N]: f32 operands, f32 accumulation, f32 result on the matrix cores
 * (csrc/gemm_f32.hip) -- the Linear layers of GroundingDINO, which the reference runs in fp32 (vlfm/vlm/grounding_dino.py:38-74,
 * groundingdino's build_model [ext]), and of MobileSAM's TinyViT (vlfm/vlm/sam.py:40-57).
 *   activation  0 none, 1 ReLU, 2 exact (erf) GELU; d_bias / d_residual may be NULL (d_residual may alias d_c)
 *   precision   0 = v_mfma_f32_32x32x2_f32: bit for bit a k-ordered f32 fma chain (157 TFLOP/s peak)
 *               1 = every operand as hi + 2^-11 lo' in two f16 (representation error <= 2^-23 |a|, one f32 ulp, for |a| >= 2^-12;
 *                   2^-36 absolute below, which is at most 2^-22 |a| on [2^-14, 2^-12)), three
 *                   f16 MFMAs per product block, f32 accumulation: f32-grade results at 5.3x the matrix rate.  Needs d_w_hi / d_w_lo
 *                   = vlfm_split_f32_to_f16_pair(d_w) (once per layer) and d_overflow, a device int that the kernel ORs with 1 when
 *                   an |operand| >= 65504 (f16's range) was met: the result of that call is then invalid and the caller must
 *                   repeat it with precision 0 (vlfm_amd/vlm/ops.py:LinearF32 does, at its next host synchronisation point)
 *   K % 32 == 0; X, W, C, residual and the split planes 16-byte aligned; M and N tails are handled. */
int vlfm_split_f32_to_f16_pair(const float* d_src, void* d_hi, void* d_lo, long long count, int* d_overflow, void* stream);
int vlfm_gemm_f32_nt(const float* d_x, const float* d_w, const float* d_bias, const float* d_residual, float* d_c, int m, int n,
                     int k, int activation, int precision, const void* d_w_hi, const void* d_w_lo, int* d_overflow, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Detector-side kernels (vlfm/vlm/yolov7.py:50-110, vlfm/vlm/grounding_dino.py:38-74)
 * ------------------------------------------------------------------------------------------- */

/* The memory-bound glue of TinyViT's windowed-attention blocks (MobileSAM's image encoder behind vlfm/vlm/sam.py:54; TinyViTBlock of
 * mobile_sam/modeling/tiny_vit_sam.py [ext]) on NHWC f32 rows (csrc/sam_ops.hip):
 *   vlfm_layernorm_rows_f32     LayerNorm over `channels` of [batch][height][width] rows; window > 0 writes the rows of the
 *                               zero-padded image in window order [batch * nWy * nWx][window^2][channels] (pad + window partition +
 *                               attn.norm in one pass; padded positions receive beta = LayerNorm(0))
 *   vlfm_window_reverse_add_f32 d_x[b][y][x][:] += d_windows[row of (b, y, x) in window order][:]  (reverse + crop + residual add)
 *   vlfm_dwconv3x3_nhwc_f32     the block's depthwise 3x3 `local_conv` (stride 1, padding 1) + folded-BatchNorm bias; d_w9c [9][channels]
 * channels % 4 == 0 everywhere. */
int vlfm_layernorm_rows_f32(const float* d_x, const float* d_gamma, const float* d_beta, float* d_out, int batch, int height,
                            int width, int channels, int window, float eps, void* stream);
int vlfm_window_reverse_add_f32(float* d_x, const float* d_windows, int batch, int height, int width, int channels, int window,
                                void* stream);
int vlfm_dwconv3x3_nhwc_f32(const float* d_x, const float* d_w9c, const float* d_bias, float* d_out, int batch, int height, int width,
                            int channels, void* stream);
/* TinyViT's window attention (head width 32; `Attention` of tiny_vit_sam.py [ext]): out = softmax(scale * q k^T + bias) v per
 * (window, head).  d_qkv [windows * tokens][heads][q | k | v][32] f32 (the qkv Linear's output), d_bias_t [heads][tokens][tokens] =
 * the additive bias TRANSPOSED (bias_t[h][j][i] = bias[h][i][j]), d_out [windows * tokens][heads * 32].  tokens <= 256. */
int vlfm_window_attention_f32(const float* d_qkv, const float* d_bias_t, float* d_out, long long windows, int tokens, int heads,
                              float scale, void* stream);
/* Swin variants (the GroundingDINO backbone, vlfm/vlm/grounding_dino.py:38-74; transformers' SwinLayer [ext]): windows of the zero-padded
 * image ROLLED by -shift along both axes (0 <= shift < window); pad_zero: padded positions receive 0 (Swin pads AFTER the norm) instead of
 * beta; d_mask_t [windows_per_image][tokens][tokens] = the shifted-window attention mask, added to window w's scores as
 * d_mask_t[w % windows_per_image] (NULL = none). */
int vlfm_layernorm_rows_shifted_f32(const float* d_x, const float* d_gamma, const float* d_beta, float* d_out, int batch, int height,
                                    int width, int channels, int window, float eps, int shift, int pad_zero, void* stream);
int vlfm_window_reverse_add_shifted_f32(float* d_x, const float* d_windows, int batch, int height, int width, int channels, int window,
                                        int shift, void* stream);
int vlfm_window_attention_masked_f32(const float* d_qkv, const float* d_bias_t, const float* d_mask_t, int windows_per_image, float* d_out,
                                     long long windows, int tokens, int heads, float scale, void* stream);

/* One convolution of the yolov7-e6e graph the reference runs in fp16 (vlfm/vlm/yolov7.py:35-48,89), BatchNorm folded:
 * out = act(conv(x, w) + bias) as an implicit GEMM on the matrix cores (csrc/conv_nhwc.hip), NHWC f16, f32 accumulation.
 *   d_x    [batch][height][width] pixels, x_pix_stride elements apart; the first `cin` channels of a pixel are read
 *   d_w    [cout][ksize][ksize][cin] (the channels_last memory of the [cout][cin][k][k] filter); d_bias [cout] or NULL
 *   d_out  [batch][Ho][Wo] pixels, out_pix_stride elements apart; `cout` channels are written (Ho = (height + 2 pad -
 *          ksize) / stride + 1, pad = ksize / 2) -- so a layer can write straight into a concatenation buffer
 *   d_zero at least 16 zero bytes in device memory (what rows in the zero padding fetch)
 *   act    0 = none, 1 = SiLU
 * ksize 1 or 3, stride 1 or 2, cin % 64 == 0, cout % 8 == 0, both pixel strides % 8 == 0, tensors < 2^31 elements;
 * anything else returns VLFM_ERR_INVALID (the caller keeps such a layer on the framework's convolution). */
/* 2x2 / stride-2 max pooling of a contiguous NHWC f16 tensor (DownC's pooling branch in the same graph): even height and width,
 * channels % 8 == 0. */
int vlfm_maxpool2x2_nhwc_f16(const void* d_x, void* d_out, int batch, int height, int width, int channels, void* stream);
int vlfm_conv_nhwc_tile(int pixels, int cin, int cout, int ksize, int* tile_pixels, int* tile_channels);  /* host: the tile shape chosen */
int vlfm_conv_nhwc_f16(const void* d_x, const void* d_w, const void* d_bias, void* d_out, const void* d_zero, int batch,
                       int height, int width, int cin, int cout, int ksize, int stride, int x_pix_stride,
                       int out_pix_stride, int act, void* stream);

/* Host: cv::computeResizeAreaTab for one axis (cv2.resize INTER_AREA, shrinking or identity).  Returns the tap count
 * used (<= ktaps_capacity) or a negative status.  h_first/h_count [dsize], h_w [dsize][ktaps_capacity]. */
int vlfm_resize_area_tab_host(int ssize, int dsize, int32_t* h_first, int32_t* h_count, float* h_w, int ktaps_capacity);

/* Device: YOLOv7.predict preprocessing (yolov7.py:70-83): d_rgb [n][H][W][3] u8 -> cv2.resize(.., (out_w, out_h),
 * INTER_AREA) -> CHW -> /255 in out_dtype (0 = f32, 1 = f16): d_out [n][3][out_h][out_w]. */
int vlfm_resize_area_batched(const uint8_t* d_rgb, int n, int height, int width, int out_h, int out_w,
                             const int32_t* d_xfirst, const int32_t* d_xcount, const float* d_xw, int xktaps,
                             const int32_t* d_yfirst, const int32_t* d_ycount, const float* d_yw, int yktaps,
                             void* d_out, int out_dtype, void* stream);

/* Device: torchvision to_tensor + normalize (grounding_dino.py:52-54): d_rgb [n][H][W][3] u8 -> d_out [n][3][H][W] f32. */
int vlfm_to_tensor_normalize_batched(const uint8_t* d_rgb, int n, int height, int width, const float* h_mean3,
                                     const float* h_std3, float* d_out, void* stream);

/* Device: torchvision.ops.nms (yolov7 non_max_suppression, yolov7.py:91-99).  d_boxes_xyxy [N][4] f32, d_order [n] int32 =
 * candidate indices sorted by descending score; d_keep [max_keep] receives the kept indices in that order, d_num_keep
 * their count.  d_scratch: vlfm_nms_scratch_bytes(n).  The whole reduction runs on the device (no host sync). */
size_t vlfm_nms_scratch_bytes(int n);
int vlfm_nms(const float* d_boxes_xyxy, const int32_t* d_order, int n, float iou_threshold, void* d_scratch,
             size_t scratch_bytes, int32_t* d_keep, int32_t* d_num_keep, int max_keep, void* stream);

/* Device: multi-scale deformable attention sampling of GroundingDINO (replaces the CUDA extension of the reference's
 * groundingdino package / its grid_sample fallback, vlfm/vlm/grounding_dino.py:14,61).  d_value [B][total][heads][D] f32,
 * d_spatial_shapes [L][2] (H,W) int32, d_level_start [L] int32, d_sampling_loc [B][Q][heads][L][P][2] in [0,1],
 * d_attn_weight [B][Q][heads][L][P] -> d_out [B][Q][heads*D].  Bilinear, zero padding, align_corners = False. */
int vlfm_ms_deform_attn(const float* d_value, const int32_t* d_spatial_shapes, const int32_t* d_level_start,
                        const float* d_sampling_loc, const float* d_attn_weight, int batch, int n_query, int n_heads,
                        int head_dim, int n_levels, int n_points, int total_len, float* d_out, void* stream);
/* The same with the softmax and the sampling-location arithmetic of GroundingDinoMultiscaleDeformableAttention.forward [ext] inside the
 * kernel: d_offsets_logits [B][Q][heads*L*P*2 + heads*L*P] = the raw output of the sampling_offsets | attention_weights Linears
 * (offsets [h][l][p][2], then logits [h][l][p]), d_reference [B][Q][L][ref_coords], ref_coords 2 (points: + offset / (W_l, H_l)) or 4
 * (boxes: + offset / P * size * 0.5).  8 heads of width 32. */
int vlfm_ms_deform_attn_fused(const float* d_value, const int32_t* d_spatial_shapes, const int32_t* d_level_start,
                              const float* d_offsets_logits, const float* d_reference, int batch, int n_query, int n_heads,
                              int head_dim, int n_levels, int n_points, int ref_coords, int total_len, float* d_out, void* stream);

/* Device: depthwise 3x3 convolution, padding 1, stride 1 or 2, NCHW f32: y = conv(x, w[C][1][3][3]) + bias[C] (NULL = none),
 * followed by the exact (erf) GELU when gelu != 0.  The depthwise convolutions of MobileSAM's TinyViT encoder behind
 * vlfm/vlm/sam.py:54 (MBConv conv2, local_conv, patch merging), with their folded BatchNorm as the bias.  width and the
 * output width must be multiples of 4. */
int vlfm_dwconv3x3_f32(const float* d_x, const float* d_w, const float* d_bias, float* d_y, int n, int channels, int height,
                       int width, int stride, int gelu, void* stream);

/* Device, in place: y[n][c][:] = act(y[n][c][:] + bias[c]) on an NCHW tensor of hw elements per plane; dtype 0 = f32, 1 = f16
 * (bias has the tensor's type); act 0 = none, 1 = exact (erf) GELU, 2 = SiLU.  The bias + activation behind every convolution
 * of the detector / MobileSAM encoders once their BatchNorm is folded into the weights (yolov7.py:70-99, sam.py:54). */
int vlfm_bias_act_nchw(void* d_y, const void* d_bias, int n, int channels, long long hw, int dtype, int act, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ObjectPointCloudMap._extract_object_cloud (vlfm/mapping/object_point_cloud_map.py:150-170,186-212) for ALL detections of a
 * step at once; a single detection is a batch of one job.  The number of kernel launches does not depend on the number of jobs.
 * ------------------------------------------------------------------------------------------- */

/* Three stages: cv2.erode(mask, None, iterations) and the point counts; valid_depth -> get_point_cloud over the eroded mask in
 * np.where order, sub-sampled by rank; open3d cluster_dbscan(eps, min_points) + "largest non-noise cluster" (:186-212).
 *
 * Stage 1, vlfm_object_cloud_batch_stats: d_masks [jobs][H][W] u8, d_erosion [jobs] i32 on the device (erosion iterations per job;
 * max_erosion = their maximum, known to the host).  d_stats [jobs][4] i32 = (points of the eroded mask, first and last occupied
 * column of the UN-eroded mask, or -1 -1 for an empty one, 0).  The eroded planes and their row offsets stay in d_scratch
 * (vlfm_object_cloud_batch_scratch_bytes(jobs, H, W)) for stage 2.
 *
 * Stage 2, vlfm_object_cloud_batch_expand: d_depth [frames][H][W] f32; d_jobs [n_jobs][6] i32 on the device = (stage-1 job,
 * depth frame, points to write, first output point, first entry of d_ranks or -1, 0).  Output point s of a job is the masked
 * pixel of np.where rank d_ranks[first + s] (or rank s without a rank list) as f64 (z, -x, -y) in d_points [capacity][3];
 * max_points = the largest "points to write".  scratch_jobs = the `jobs` of the stage-1 call that filled d_scratch.
 *
 * Stage 3, vlfm_dbscan_largest_cluster_batch: d_jobs [n_jobs][3] i64 on the device = (n, first point in d_points, byte offset of
 * the job's scratch: a multiple of 256, vlfm_dbscan_batch_scratch_bytes(n) bytes); max_n = the largest n (<= 8192).  The points
 * of job j's largest cluster are written in order to d_kept at the job's own first point, their number to d_num_keep[j]
 * (0 = only noise, or n == 0).
 * After the call a job's scratch holds, behind its n * ceil(n / 64) adjacency words (u64; bit j of word (i, cb) = point 64 cb + j
 * lies within eps of point i), four [n] i32 arrays: degree, sizes, label, keep.  label = the cluster root index of every point
 * (INT32_MAX = noise); keep[0 : d_num_keep[j]] = the indices of the largest cluster in ascending order.
 *
 * vlfm_object_cloud_launch_count: kernels launched so far by every function of this section (diagnostics, tests). */
size_t vlfm_object_cloud_batch_scratch_bytes(int jobs, int height, int width);
int vlfm_object_cloud_batch_stats(const uint8_t* d_masks, const int32_t* d_erosion, int jobs, int max_erosion, int height, int width,
                                  void* d_scratch, int32_t* d_stats, void* stream);
int vlfm_object_cloud_batch_expand(const float* d_depth, int frames, int height, int width, double min_depth, double max_depth,
                                   double fx, double fy, const void* d_scratch, int scratch_jobs, const int32_t* d_jobs, int n_jobs,
                                   int max_points, const int32_t* d_ranks, int n_ranks, double* d_points, int capacity, void* stream);
size_t vlfm_dbscan_batch_scratch_bytes(int n);
int vlfm_dbscan_largest_cluster_batch(const double* d_points, int capacity, const int64_t* d_jobs, int n_jobs, int max_n, double eps,
                                      int min_points, void* d_scratch, size_t scratch_bytes, double* d_kept, int32_t* d_num_keep,
                                      void* stream);
long long vlfm_object_cloud_launch_count(void);

/* ---------------------------------------------------------------------------------------------
 * Queries over device mirrors of the accumulated object clouds (ABI 18, csrc/cloud_query.hip): what
 * ObjectPointCloudMap.update_explored and get_best_object ask of a cloud (object_point_cloud_map.py:77-144,172-183,
 * geometry_utils.py:91-116), for many clouds in one launch.  The number of launches does not depend on the number of queries.
 * ------------------------------------------------------------------------------------------- */

/* One query = one cloud.  d_rows [n][4] f64 (x, y, z, tag), 32-byte aligned; d_slots [n] i32: -1 for a point whose tag is 1.0,
 * else the index (< n_slots) of its tag in the caller's table of the cloud's other tag values.  p = the cone's origin (cone) or
 * the position (closest: its first k entries, k = 2 or 3).  heading, half_fov (= cone_fov / 2), range: the cone; flag_offset:
 * where the cloud's 2 * n_slots flags start in d_flags. */
typedef struct {
    const double* d_rows;
    const int32_t* d_slots;
    double p[3];
    double heading, half_fov, range;
    int32_t n, k, flag_offset, n_slots;
} vlfm_cloud_query;

/* d_flags (zeroed by the caller) [flag_offset + s] = 1 when slot s has a point with dist <= range and |angle diff| <= half_fov,
 * [flag_offset + n_slots + s] = 1 when it has a point with dist <= range whose |angle diff| lies within 1e-9 rad of half_fov:
 * such a point is UNCERTAIN (the device's atan2 is not NumPy's) and is counted on neither side; the caller decides it.  Points of
 * slot -1 are skipped.  max_points = the largest n.  One launch. */
int vlfm_cloud_cone_flags(const vlfm_cloud_query* d_queries, int n_queries, int max_points, int32_t* d_flags, void* stream);

/* d_result [n_queries][4] i32 = (points with tag 1.0, np.argmin of norm(rows[:, :k] - p) over those points as an index into the
 * WHOLE cloud or -1 when there is none, the same over all points or -1 for an empty cloud, 0).  The minimum is taken over the
 * rounded roots; ties go to the lowest index.  Two launches: per-chunk partials into d_scratch
 * (vlfm_cloud_closest_scratch_bytes(n_queries, max_points)), then one wavefront per query. */
size_t vlfm_cloud_closest_scratch_bytes(int n_queries, int max_points);
int vlfm_cloud_closest(const vlfm_cloud_query* d_queries, int n_queries, int max_points, void* d_scratch, size_t scratch_bytes,
                       int32_t* d_result, void* stream);
/* points per workgroup chunk; kernels launched so far by the functions of this section */
int vlfm_cloud_query_chunk(void);
long long vlfm_cloud_query_launch_count(void);

/* ---------------------------------------------------------------------------------------------
 * ObstacleMap planes are bit-packed: 1 bit per cell, row stride ceil(cols/32) u32 words, bit x&31 of word x>>5.
 * ------------------------------------------------------------------------------------------- */
int vlfm_bits_pack(const uint8_t* d_src, uint32_t* d_dst, int planes, int rows, int cols, void* stream);
int vlfm_bits_unpack(const uint32_t* d_src, uint8_t* d_dst, int planes, int rows, int cols, void* stream);

/* cv2.dilate(img, ones((kernel_h, kernel_w))) on packed planes (odd sizes, anchor centre, border ignored)
 * (obstacle_map.py:105-109,125,159-163). */
int vlfm_bits_dilate(const uint32_t* d_src, uint32_t* d_dst, int planes, int rows, int cols, int kernel_w,
                     int kernel_h, void* stream);

/* cv2.findContours(img, RETR_EXTERNAL, method) (obstacle_map.py:128-132) on packed planes, one wavefront per plane.
 * method 1 = CHAIN_APPROX_NONE, 2 = CHAIN_APPROX_SIMPLE.  Outputs per plane: d_pts [cap_pts][2] (x,y) in DISCOVERY
 * order (OpenCV returns the reverse), d_starts/d_lens [cap_contours], d_counts [3] = (contours, points, overflow). */
int vlfm_find_contours_external(const uint32_t* d_img, int planes, int rows, int cols, int method,
                                uint32_t* d_scratch /* [2][planes][rows][stride] */, int32_t* d_pts, int cap_pts,
                                int32_t* d_starts, int32_t* d_lens, int cap_contours, int32_t* d_counts, void* stream);

/* The same result from ONE 1024-thread workgroup per plane (csrc/border_parallel.h: successor tables + list ranking on a padded
 * LDS copy) -- the form the obstacle-map kernels use on their windows.  The plane must fit the LDS window
 * (3 * (rows + 2) * ((ceil(cols/32) + 2) | 1) * 4 <= 144 KB and rows * ceil(cols/32) <= 65535), else VLFM_ERR_CAPACITY.
 * d_scratch: vlfm_find_contours_wg_scratch_bytes(...) bytes.  method | 0x100 keeps the follower's tables in global memory (the
 * fallback form of the map kernels, for windows whose tables do not fit the LDS behind the window planes); without the flag the
 * tables live in LDS and every border of the plane is ranked at once (the form the map kernels use when it fits).
 * vlfm_walk_path_counters: how the borders of all launches so far were traced -- h_out4 = (borders from the ranked tables, planes /
 * windows whose per-pixel tables were in global memory (large windows), borders walked by one lane although the ranked tables
 * existed, planes / windows with every table in LDS); reset != 0 zeroes them. */
size_t vlfm_find_contours_wg_scratch_bytes(int planes, int rows, int cols, int cap_pts);
int vlfm_walk_path_counters(long long* h_out4, int reset);
int vlfm_find_contours_external_wg(const uint32_t* d_img, int planes, int rows, int cols, int method, void* d_scratch,
                                   size_t scratch_bytes, int32_t* d_pts, int cap_pts, int32_t* d_starts, int32_t* d_lens,
                                   int cap_contours, int32_t* d_counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * ObstacleMap.update_map, explore half (obstacle_map.py:105-169) for n environments.
 * ------------------------------------------------------------------------------------------- */
#define VLFM_FOG_MAX_POLY 80
typedef struct {
    int32_t env;            /* plane slot */
    int32_t ax, ay;         /* agent cell (x = col, y = row) = BaseMap._xy_to_px(tf[:2,3]) (obstacle_map.py:115-116) */
    int32_t radius;         /* int(max_line_len) = int(max_depth * ppm) */
    int32_t n_poly;         /* vertices in poly; 0 = this environment is skipped */
    int32_t reserved;
    double rot_c, rot_s;    /* cos/sin(-angle_cv2) as reveal_fog_of_war's get_two_farthest_points evaluates them [ext] */
    double line_len;        /* max_line_len * 1.05 */
    long long poly[2 * VLFM_FOG_MAX_POLY]; /* 16.16 fixed-point FOV sector polygon (cv2.ellipse), image coordinates */
} vlfm_fog_params;

/* Host: fills vlfm_fog_params for n environments.  h_agent_px [n][2] (x,y) cells; h_angle_cv2_deg [n] =
 * rad2deg(wrap_heading(yaw + pi/2)); h_rot_cs [n][2]; sector = cv2.ellipse(centre, (R,R), 0, a - fov/2, a + fov/2). */
int vlfm_fog_params_host(const int32_t* h_agent_px, const double* h_angle_cv2_deg, const double* h_rot_cs,
                         double fov_deg, double max_line_len, const int32_t* h_env, const int32_t* h_explore, int n,
                         vlfm_fog_params* h_out);

size_t vlfm_obstacle_scratch_bytes(int n_envs, int map_size, int cap_pts, int cap_contours);

/* Device pipeline: [navigable = ~dilate(obstacle, k x k); explored &= navigable] -> fog of war reveal -> explored
 * component selection -> frontier midpoints.
 *   d_obstacle/d_navigable/d_explored  [n_envs][S][stride] bit-packed planes
 *   d_bbox      [n_envs][4] int32 persistent (ymin, ymax, xmin, xmax) of everything ever revealed; reset value
 *               (S, -1, S, -1)
 *   d_frontiers [n_envs][cap_frontiers][2] f64 pixel coordinates (x, y) == ObstacleMap._frontiers_px
 *   d_counts    [n_envs][4] int32: (n frontiers, overflow flag, n contours, n chain points)
 *   d_windows   [n][12] int32 or NULL.  Per observation three inclusive cell windows (y0, y1, x0, x1; empty when y1 < y0):
 *               [0..3] where `navigable` has to be recomputed = the union of the reach windows (camera cell +- the largest
 *               distance a scattered texel can have, + 1) of every frame ingested into this slot since its last call with
 *               update_obstacles, grown by kernel_size / 2; [4..7] where `explored` has to be masked = the caller's mirror
 *               of d_bbox BEFORE this call (no explored bit exists outside it); [8..11] where the frontier stage's derived
 *               planes are refreshed = the windows [0..3] of every call since this slot's last call with explore, united
 *               with d_bbox AFTER this call's reveal (agent cell +- (fog_radius + 2), clipped) grown by 3.  The caller
 *               passes the whole map (0, S-1, 0, S-1) after a reset of the slot's planes, for a frame whose reach window
 *               leaves the map (NumPy's negative-index wrap, obstacle_map.py:101, lands on the far side) and for the first
 *               call on fresh scratch.  NULL = the reference's full-map passes (always valid).
 *               SKIPPED observations (d_prm[k].n_poly <= 0): the kernels neither mask nor refresh anything for them, so the
 *               caller must KEEP that observation's pending windows [0..3] / [8..11] in its own bookkeeping and hand them
 *               over again with the slot's next non-skipped call (ObstacleMapBatch._take_windows does); dropping them leaves
 *               stale derived planes and stale frontiers.
 *   window_blocks_navigable / window_blocks_prepare: launch sizes (256-word workgroups per observation) for the two windowed
 *               kernels = ceil(max over the batch of rows x 32-cell words of the window(s) / 256); the kernels stride, so
 *               any positive value is correct and 0 means "size for the full plane". */
int vlfm_obstacle_map_update_batched(const vlfm_fog_params* d_prm, int n, const uint32_t* d_obstacle,
                                     uint32_t* d_navigable, uint32_t* d_explored, int32_t* d_bbox, int n_envs,
                                     int map_size, int kernel_size, int fog_radius, double area_thresh_px,
                                     void* d_scratch, size_t scratch_bytes, int cap_pts, int cap_contours,
                                     double* d_frontiers, int cap_frontiers, int32_t* d_counts, int update_obstacles,
                                     int explore, const int32_t* d_windows, int window_blocks_navigable,
                                     int window_blocks_prepare, void* stream);

/* Debug/diagnostic: copies the per-environment status words of the last pipeline run to the host. */
int vlfm_obstacle_status(const void* d_scratch, int n_envs, int map_size, int cap_pts, int cap_contours,
                         int32_t* h_out);

/* ---------------------------------------------------------------------------------------------
 * Map rendering: ValueMap.visualize (value_map.py:189-219 + img_utils.py:64-85) and ObstacleMap.visualize
 * (obstacle_map.py:171-192) with the TrajectoryVisualizer overlay (traj_visualizer.py), for n frames at once, into a
 * caller-given uint8 [n][S][S][3] buffer (BGR like the reference; rgb != 0 swaps B and R).
 *
 * d_frames [n][4] int32 per frame: (env slot, 1 = the slot's `_value_map` is f32 (normalise in f32) / 0 = f64,
 *          explored plane index into d_explored or -1 = no explored mask, 0).
 * Primitives: d_prim_off [n+1] int32 ranges into d_prims, one frame's primitives in drawing order; d_vtx [..][2] int64
 *          16.16 vertices of VLFM_PRIM_POLYLINE.  d_prims = NULL: no primitives.
 * d_path   [n_envs][S][stride] trajectory bit-planes in IMAGE coordinates (after the flip), or NULL.
 * ------------------------------------------------------------------------------------------- */
enum { VLFM_REDUCE_MAX = 0,        /* np.max(value, axis=-1) (value_map.py:192) */
       VLFM_REDUCE_EXPLORE = 1,    /* np.where(v[..., 0] > t, v[..., 0], max) (ITMPolicyV3, itm_policy.py:275-287) */
       VLFM_REDUCE_PLANE = 2 };    /* d_plane [n][S][S] f64: reduced on the host by any other reduce_fn */
enum { VLFM_PRIM_CIRCLE_FILL = 0,  /* cv2.circle(thickness < 0): midpoint fill; x0,y0 centre, x1 radius */
       VLFM_PRIM_CIRCLE = 1,       /* cv2.circle(thickness 0 or 1): midpoint outline */
       VLFM_PRIM_LINE = 2,         /* cv2.line(x0,y0 -> x1,y1, thickness >= 2): ThickLine with both caps */
       VLFM_PRIM_POLYLINE = 3 };   /* cv2.circle(thickness > 1): EllipseEx's open PolyLine over n_vtx 16.16 vertices */
#define VLFM_RENDER_FLIP_ROWS 1    /* drawn before the frame's vertical flip (ObstacleMap's frontier circles) */
#define VLFM_RENDER_UNDER_PATH 2   /* drawn before the trajectory: pixels of the path plane keep the path colour */
typedef struct {
    int32_t frame;                 /* informational: the frame whose range holds this primitive */
    int32_t kind;                  /* VLFM_PRIM_* */
    int32_t flags;                 /* VLFM_RENDER_* */
    int32_t thickness;
    int32_t x0, y0, x1, y1;        /* image coordinates (x = column, y = row) */
    int32_t vtx_off, n_vtx;        /* VLFM_PRIM_POLYLINE vertices in d_vtx */
    uint8_t bgr[4];
    int32_t reserved;
} vlfm_render_prim;                /* 48 bytes */

size_t vlfm_value_render_scratch_bytes(int n, int map_size);

/* d_value [n_envs][S][S][channels] f64 (ValueMapBatch.value); d_explored [*][S][stride] or NULL. */
int vlfm_value_map_render(const double* d_value, int n_envs, int map_size, int channels, const int32_t* d_frames, int n,
                          int reduce_mode, double explore_thresh, const double* d_plane, const uint32_t* d_explored,
                          const uint32_t* d_path, const int32_t* d_prim_off, const vlfm_render_prim* d_prims,
                          const int64_t* d_vtx, int rgb, void* d_scratch, size_t scratch_bytes, uint8_t* d_out,
                          void* stream);

/* d_obstacle / d_navigable / d_explored [n_envs][S][stride]; pad_bgr = radius_padding_color packed b | g << 8 | r << 16. */
int vlfm_obstacle_map_render(const uint32_t* d_obstacle, const uint32_t* d_navigable, const uint32_t* d_explored,
                             int n_envs, int map_size, const int32_t* d_frames, int n, uint32_t pad_bgr,
                             const uint32_t* d_path, const int32_t* d_prim_off, const vlfm_render_prim* d_prims,
                             const int64_t* d_vtx, int rgb, uint8_t* d_out, void* stream);

/* ORs m trajectory segments d_segs [m][5] int32 (env slot, x0, y0, x1, y1) into d_path [n_envs][S][stride] as
 * cv2.line(mask, p0, p1, 255, thickness) draws them (traj_visualizer.py:60-80); thickness >= 2. */
int vlfm_traj_append(uint32_t* d_path, int n_envs, int map_size, const int32_t* d_segs, int m, int thickness,
                     void* stream);

/* Host: the 16.16 vertices EllipseEx hands to PolyLine for cv2.circle(centre, radius, thickness > 1) -- ellipse2Poly
 * over 0..360 from OpenCV's float sine table, snapped, duplicates dropped (the sector code of vlfm_fog_params_host).
 * h_circles [n][3] (cx, cy, radius); vertices of circle i are h_xy[2*h_off[i] ..] with h_off [n+1]. */
int vlfm_circle_polygon_host(const int32_t* h_circles, int n, int64_t* h_xy, int32_t* h_off, int capacity);

/* ---------------------------------------------------------------------------------------------
 * JPEG transport emulation: the reference's client -> server hop (server_wrapper.py:57-68: cv2.imencode at quality q,
 * then cv2.imdecode) for n frames at once.  d_in / d_out are uint8 [n][H][W][3] device frames packed back to back, in the
 * slot order the reference hands cv2 (slot 2 is read as R, slot 0 as B); each output frame is bit-identical to Pillow's
 * libjpeg-turbo baseline 4:2:0 encode + decode of that frame (vlfm_amd/vlm/transport.py:jpeg_roundtrip).  No bit stream
 * is formed: the quantised coefficients stay on the chip.  d_out may be d_in (the input is read in full before the first
 * output byte is written).  h_tables [2][64] host: luma, chroma quantisation tables in natural order, entries 1..255
 * (vlfm_jpeg_quant_tables_host).  d_scratch: 16-byte aligned device buffer of vlfm_jpeg_scratch_bytes(n, H, W) bytes
 * (decoded Y, Cb, Cr planes), not overlapping d_in / d_out.  1 <= H, W <= 65500 (JPEG_MAX_DIMENSION).
 * ------------------------------------------------------------------------------------------- */
int vlfm_jpeg_quant_tables_host(int quality, uint16_t* h_tables);   /* jcparam.c jpeg_set_quality(quality, TRUE) */
size_t vlfm_jpeg_scratch_bytes(int n, int H, int W);               /* 0 for invalid sizes */
int vlfm_jpeg_roundtrip_batched(const uint8_t* d_in, uint8_t* d_out, int n, int H, int W, const uint16_t* h_tables,
                                void* d_scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * JPEG encoder (ABI 12): the files Pillow's save(format="JPEG", quality=q, subsampling="4:2:0") writes through
 * libjpeg-turbo, byte for byte, for n frames at once: baseline, one interleaved scan, the standard Huffman tables of
 * Annex K, no restart markers (csrc/jpeg_entropy.hip; tests/jpeg_huff_ref.py is the NumPy form).
 *
 * vlfm_jpeg_header_host: the 623 bytes in front of the scan (SOI, APP0 JFIF 1.01, two DQT, SOF0, four DHT, SOS) for
 *   (quality, H, W); *len = 623 always, VLFM_ERR_CAPACITY if cap is less.
 * vlfm_jpeg_encode_bound: a capacity no frame of H x W can exceed, whatever its content and tables; 0 for sizes the encoder
 *   does not take.  Derivation: a block costs at most one DC code of 11 bits + 11 amplitude bits and, for each of its 63
 *   AC coefficients, a 16-bit run/size code + 10 amplitude bits (a ZRL or EOB code replaces >= 1 such coefficient and is
 *   shorter): 1660 bits.  bound = 623 + 2 * ceil(6 * ceil(H/16) * ceil(W/16) * 1660 / 8) + 2: the header, the scan with
 *   its last byte padded and every byte stuffed, EOI.
 * vlfm_jpeg_encode_scratch_bytes: the scratch the call below needs (coefficients, block bit offsets, the unstuffed stream at
 *   the bound, 0xFF counts); 0 for invalid sizes.
 * vlfm_jpeg_encode_batched: d_in uint8 [n][H][W][3] device frames packed back to back; rgb_order 0 reads slot 2 of a pixel
 *   as R (what cv2.imencode does with the frame the reference hands it: the convention of vlfm_jpeg_roundtrip_batched),
 *   1 reads slot 0 as R (Image.fromarray(rgb).save).  Frame i's file goes to d_out + i * capacity, its full length to
 *   d_lengths[i].  A frame longer than capacity is cut at capacity -- no byte outside its own slot is written, the other
 *   frames are complete, the call still returns VLFM_OK and d_lengths[i] > capacity tells.  Bytes of a slot behind the
 *   file's end are left as they were.  h_tables, d_scratch alignment and the argument checks as for the round trip; in
 *   addition frames whose scan could pass 2^32 bits (6 * ceil(H/16) * ceil(W/16) * 1660 >= 2^32, about 10 000 x 10 000
 *   pixels) are refused: bit offsets and lengths are 32-bit.  Seven kernel launches on `stream`, no synchronisation.
 * ------------------------------------------------------------------------------------------- */
int vlfm_jpeg_header_host(int quality, int H, int W, uint8_t* h_out, size_t cap, size_t* len);
size_t vlfm_jpeg_encode_bound(int H, int W);
size_t vlfm_jpeg_encode_scratch_bytes(int n, int H, int W);
int vlfm_jpeg_encode_batched(const uint8_t* d_in, int n, int H, int W, int rgb_order, const uint16_t* h_tables,
                             uint8_t* d_out, size_t capacity, uint32_t* d_lengths, void* d_scratch, size_t scratch_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * JPEG decoder (ABI 14): n baseline 4:2:0 files of one H x W to uint8 [n][H][W][3] device frames, bit-equal to libjpeg-turbo
 * as Pillow drives it (Image.open(...).convert("RGB")) for files an encoder made from 8-bit pixels (csrc/jpeg_decode.hip;
 * tests/jpeg_dec_ref.py is the NumPy form).  Accepted: SOF0, 8-bit samples, three components sampled 2x2, 1x1, 1x1 with any
 * ids and table selectors, one interleaved scan, 8-bit quantisation tables, the file's own Huffman tables (Annex K's or
 * optimised), any restart interval; APPn (but Adobe APP14) and COM segments and 0xFF fill bytes are skipped.
 *
 * vlfm_jpeg_parse_host: walks the markers of one file up to the scan.  Fills *frame (table_set = 0) and *set: per component
 *   (Y, Cb, Cr) the quantisation table in natural order and the DC and AC Huffman tables in canonical-compare form: a
 *   left-aligned 16-bit window x has code length 1 + #{l : x >= limit[l]} (17: no such code), and its symbol is
 *   vals[(x >> (16 - len)) - delta[len - 1]].  Returns VLFM_OK, VLFM_ERR_INVALID for a null argument, or a positive reason
 *   code for a file the decoder does not take; vlfm_jpeg_parse_reason gives its text.  A prefix of a file that ends behind
 *   SOS parses like the file (this is how the header of the device form below is read).
 * vlfm_jpeg_decode_chunk_bytes: the bytes of a file one workgroup of the marker scan takes; chunk c is file bytes
 *   [c * chunk, (c + 1) * chunk).
 * vlfm_jpeg_decode_scratch_bytes: the scratch the call below needs; 0 for invalid sizes.  Its first
 *   n * ceil(H/16) * ceil(W/16) * 768 bytes are, after the call, the coefficients of the scan in the encoder's layout: 64 int16
 *   per block in zigzag order, blocks in scan order (MCUs row-major; Y00 Y01 Y10 Y11 Cb Cr), absolute DC values.
 * vlfm_jpeg_decode_batched: file i is the d_lengths[i] bytes (device int32) at d_files + d_offsets[i] (device int64), or,
 *   with d_offsets null, at d_files + i * stride; no byte outside [d_files, d_files + files_bytes) or, without offsets, outside
 *   the file's stride is read whatever the lengths say, and at most max_file_bytes of a file.  d_frames [n] and d_sets
 *   [n_sets] are device copies of what vlfm_jpeg_parse_host filled, table_set indexing d_sets.  d_header, if not null, is a
 *   device copy of the header_bytes every file must start with (compared on the device).  max_segments >= the largest
 *   ceil(MCUs / restart_interval) of the batch (1 for files without restart markers).  rgb_order 0 writes R to slot 2 of a
 *   pixel (cv2.imdecode's BGR, the convention of vlfm_jpeg_roundtrip_batched), 1 to slot 0.  d_status int32 [n]: 0 for a
 *   good frame, else the largest of the VLFM_JPEG_BAD_* codes the stream ran into; such a frame's pixels are unspecified, every other
 *   frame is complete, and nothing outside d_out, d_status and d_scratch is written: every index formed from stream bits is
 *   range-checked or clamped before use.  Surplus bits behind a segment's last MCU are accepted.  Six kernel launches and
 *   one memset on `stream`, no synchronisation; every grid is sized from n, the MCU count, max_segments and max_file_bytes.
 * ------------------------------------------------------------------------------------------- */
typedef struct vlfm_jpeg_huff {
    uint32_t limit[16];
    int32_t delta[16];
    uint8_t vals[256];
} vlfm_jpeg_huff;                                   /* 384 bytes */
typedef struct vlfm_jpeg_table_set {
    uint16_t quant[3][64];
    vlfm_jpeg_huff dc[3];
    vlfm_jpeg_huff ac[3];
} vlfm_jpeg_table_set;                              /* 2688 bytes */
typedef struct vlfm_jpeg_frame {
    int32_t height, width, restart_interval, scan_offset, table_set, reserved[3];
} vlfm_jpeg_frame;                                  /* 32 bytes */
enum {
    VLFM_JPEG_BAD_HEADER = 1,      /* device form: the file does not start with the given header */
    VLFM_JPEG_BAD_LENGTH = 2,      /* the file ends at or before the first byte of its scan */
    VLFM_JPEG_BAD_EOI = 3,         /* no EOI behind the scan (or another marker first) */
    VLFM_JPEG_BAD_RESTART = 4,     /* RSTn out of order, or not ceil(MCUs / Ri) - 1 of them */
    VLFM_JPEG_BAD_CODE = 5,        /* a bit pattern that is no code of the table in force */
    VLFM_JPEG_BAD_SIZE = 6,        /* a DC size above 11 or an AC size above 10 */
    VLFM_JPEG_BAD_INDEX = 7,       /* a run that passes zigzag index 63 */
    VLFM_JPEG_BAD_BITS = 8         /* a segment out of bits before its MCUs are complete */
};
int vlfm_jpeg_parse_host(const uint8_t* h_file, size_t len, vlfm_jpeg_frame* frame, vlfm_jpeg_table_set* set);
const char* vlfm_jpeg_parse_reason(int code);
size_t vlfm_jpeg_decode_chunk_bytes(void);
size_t vlfm_jpeg_decode_scratch_bytes(int n, int H, int W, size_t max_file_bytes);
int vlfm_jpeg_decode_batched(const uint8_t* d_files, size_t files_bytes, const int64_t* d_offsets, size_t stride,
                             const int32_t* d_lengths, int n, int H, int W, const vlfm_jpeg_frame* d_frames,
                             const vlfm_jpeg_table_set* d_sets, int n_sets, const uint8_t* d_header, int header_bytes,
                             int max_segments, size_t max_file_bytes, int rgb_order, uint8_t* d_out, int32_t* d_status,
                             void* d_scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Synthetic worlds (ABI 24, csrc/world_render.hip): what n cameras see in worlds of axis-aligned boxes, ray-cast per image
 * column in ONE launch.  Test-world infrastructure of the batched harness (the reference observes through Habitat): it lets a
 * closed-loop episode render from wherever the robot's own actions took it.
 *
 * The world table: every camera (and every geodesic field, below) stands in one row of a table of floor plans
 * (vlfm_amd.harness.WorldTable keeps it, synthetic.ProceduralWorlds generates plans).  The fixed rooms world (synthetic.BOXES) is
 * a table of one row with max_boxes = its box count.
 *   d_world_boxes  [n_worlds][max_boxes][4] doubles: x0, y0, x1, y1
 *   d_box_counts   [n_worlds] int32: the boxes of each world, clamped to [0, max_boxes] by the kernels; rows beyond a world's
 *                  count are never read as boxes, whatever they hold
 *   d_world_of     [n] int32: the world (row of the table) of each camera / field.  An index outside [0, n_worlds) is an EMPTY
 *                  world; the kernels never read out of bounds for it (the Python wrappers refuse it before any launch).
 * A workgroup stages the `count` boxes of its camera's world; max_boxes sizes the LDS layout and the output strides.
 *
 * vlfm_worlds_raycast, on `stream`:
 *   d_cameras  n records of 8 doubles (64 bytes): x, y, cos(yaw), sin(yaw), camera height, fx (pixels), min_depth, max_depth
 *              (max_depth > min_depth: the frame is normalised to that range and clamped to [1e-3, 1])
 *   d_depth    [n][H][W] float
 * d_objects == NULL: walls only.  Bit for bit synthetic.render_objects_numpy(..., boxes6 = [], boxes = the world's boxes)[0] in
 * NumPy and, for the tabulated headings, synthetic.depth_from_profile(synthetic.wall_profile(..., boxes = the world's boxes)).
 * d_env_of, n_envs, d_ids, d_stats and the colour arguments are ignored; d_rgb must be NULL.  max_boxes, one image row
 * and one band of rows must fit 64 KB of LDS.
 *
 * d_objects set: up to 8 objects per environment -- axis-aligned boxes with a vertical extent -- stand in front of the walls,
 * rendered with occlusion (plus a fill of d_stats), bit for bit synthetic.render_objects_numpy(..., boxes = the world's boxes) /
 * object_stats_numpy.
 *   d_objects  [n_envs][8][8] doubles: x0, y0, x1, y1, z0, z1, valid (0 = no object in this slot), pad
 *   d_env_of   [n] the environment (row of d_objects) each camera looks at, in [0, n_envs) (checked by the caller: the
 *              kernel treats anything else as "no objects")
 *   d_ids      [n][H][W] uint8: 0 = wall / floor, k + 1 = object slot k
 *   d_stats    [n][8][5] int32 per object slot: visible pixels, first / last column, first / last row;
 *              (0, W, -1, H, -1) for an object without a pixel
 * Per column u an object is hit by the walls' slab test at t = f64(f32(tmin)) and covers the rows r with
 * ceil((height - z1) fx / t) <= r - H/2 <= floor((height - z0) fx / t); a pixel takes the f32 minimum of wall, floor and
 * the covering objects, and the id of the nearest covering object (lowest slot among equals) where that is STRICTLY nearer
 * than wall and floor.  max_boxes, 69 bytes per image column and one band of rows must fit 64 KB of LDS; n_envs >= 1, H <= 32768.
 *
 * d_objects and d_rgb set: the camera's RGB view of the same world as well, from the same launch, every byte what
 * synthetic.render_rgb_numpy computes; d_depth, d_ids and d_stats are bit for bit those without d_rgb.  d_rgb without d_objects
 * is refused; a world without objects is an object row of zeros.  Colours are packed 0x00RRGGBB (the top byte is ignored).
 *   d_object_colours  [n_envs][8] int32: the colour of each object slot of d_objects (required with d_rgb)
 *   d_palette         [12] int32: 8 wall colours, 2 floor colours, the void, one spare entry (required with d_rgb)
 *   d_rgb             [n][H][W][3] uint8: R, G, B
 * Per column: the wall is the box b_w with the least tmin among the hit boxes (lowest index among equals, counted inside the
 * camera's own world) at t_w = f64(f32(tmin)); it shows a y-face iff min(ty0, ty1) > min(tx0, tx1); q = x + dx t_w on a y-face,
 * y + dy t_w on an x-face; panel = floor(2 q) & 1; r_sk = ceil(((height - 0.12) fx) / t_w) clamped to int16.  Per pixel, with
 * rr = r - H/2, the first that holds:
 *   object  id > 0: the slot's colour; its footprint shows a y-face: ch -= ch >> 2
 *   floor   floor_d < t_w (f64): palette[8 + ((floor(2 px) + floor(2 py)) & 1)], (px, py) = (x, y) + (dx, dy) floor_d
 *   wall    t_w finite: palette[mix32(b_w, 0, 31) % 8]; an odd panel: ch -= ch >> 3; a y-face: ch -= ch >> 2; rr >= r_sk: ch >>= 1
 *   void    palette[10], as it is
 * and on the first three the depth cue g = int(depth * 128.0f), ch = (ch * (256 - g)) >> 8.  One rounding per f64 operation.
 * max_boxes, 95 bytes per image column and one band of at most 128 rows (12 bytes each) must fit 64 KB of LDS.
 *
 * n <= 65535; anything refused above is VLFM_ERR_INVALID, nothing launched, nothing written; n == 0 returns VLFM_OK. */
int vlfm_worlds_raycast(const double* d_cameras, int n, const double* d_world_boxes, const int32_t* d_box_counts, int n_worlds,
                        int max_boxes, const int32_t* d_world_of, const double* d_objects, const int32_t* d_env_of, int n_envs,
                        int H, int W, float* d_depth, uint8_t* d_ids, int32_t* d_stats, const int32_t* d_object_colours,
                        const int32_t* d_palette, uint8_t* d_rgb, void* stream);

/* Grid worlds (ABI 25): a world of the table may also hold an OCCUPANCY GRID -- a top-down map of up to 1024 x 1024 cells whose
 * occupied cells are full-height walls (vlfm_amd.synthetic.GridPlan).  A grid world IS the box world of its occupied cells:
 * cell (i, j) is the box (xs[i], ys[j], xs[i+1], ys[j+1]), and depth, ids and stats are bit for bit what the box statements give
 * for those boxes (closed slabs, tmin > 0: a cell around the camera is transparent, |dx| < 1e-12 -> 1e-12).  A world with boxes
 * AND a grid: the wall of a column is the f64 minimum of the two, rounded to f32 after.  The kernels do not loop over cells:
 * per column a grid walk over the slab test's own crossing times (csrc/world_render.hip: grid_walk; the host statement is
 * synthetic.grid_profile_numpy) gives the same bits in at most nx + ny + 2 steps.
 *   d_grid_bits   [n_worlds][max_ny][ceil(max_nx / 32)] uint32: bit i % 32 of word i / 32 of row j: cell (i, j) is a wall
 *   d_grid_edges  [n_worlds][max_nx + 1 + max_ny + 1] doubles: xs (nx + 1 of them, strictly increasing), then, from index
 *                 max_nx + 1, ys (ny + 1)
 *   d_grid_dims   [n_worlds][2] int32: ny, nx, clamped to [0, max_ny] and [0, max_nx] by the kernels; a zero: the world has no
 *                 grid.  Cells and edges beyond a world's dims are never read, whatever the table holds there.
 * vlfm_worlds_raycast_grids is vlfm_worlds_raycast with these arrays -- all three, or all three NULL, which IS
 * vlfm_worlds_raycast (max_nx, max_ny ignored).  With grids: max_nx and max_ny in [1, VLFM_GRID_MAX_CELLS], and d_rgb must be
 * NULL (wall colours are defined by box and face); anything else is VLFM_ERR_INVALID, nothing launched, nothing written.  Bits
 * and edges are read from global memory; the LDS needs are those above. */
#define VLFM_GRID_MAX_CELLS 1024
int vlfm_worlds_raycast_grids(const double* d_cameras, int n, const double* d_world_boxes, const int32_t* d_box_counts,
                              int n_worlds, int max_boxes, const int32_t* d_world_of, const double* d_objects,
                              const int32_t* d_env_of, int n_envs, int H, int W, float* d_depth, uint8_t* d_ids, int32_t* d_stats,
                              const int32_t* d_object_colours, const int32_t* d_palette, uint8_t* d_rgb,
                              const uint32_t* d_grid_bits, const double* d_grid_edges, const int32_t* d_grid_dims, int max_nx,
                              int max_ny, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Geodesic distances in the synthetic worlds (ABI 19; the fields read the world table since ABI 24; csrc/geodesic.hip): the
 * length of the shortest collision-free path from a point to an ObjectNav goal, which SPL, SoftSPL and distance_to_goal are made of (the reference reads them off Habitat's
 * navmesh).  Bit for bit vlfm_amd.synthetic.geodesic_field_numpy / geodesic_query_numpy: f64, one rounding per operation,
 * no fused multiply-add, the expressions as written here.
 *   rectangles  the `count` wall boxes (x0, y0, x1, y1) of the field's world, then the environment's object slots with
 *               valid != 0 in slot order -- synthetic.inflated_rects(objects, margin, boxes) --, each inflated to
 *               (x0 - margin, y0 - margin, x1 + margin, y1 + margin).  OPEN sets.
 *   blocked     the segment p -> q is blocked by a rectangle iff some t in (0, 1) puts p + t (q - p) strictly inside it:
 *               per axis, with d = q - p:  d == 0: the interval is (-inf, inf) if lo < p < hi, else empty;  otherwise
 *               t0 = (lo - p) / d, t1 = (hi - p) / d, interval (min(t0, t1), max(t0, t1));
 *               blocked iff max(enter_x, enter_y, 0) < min(exit_x, exit_y, 1).  A segment along an edge or through a corner
 *               is free.  Evaluated from p to q: source -> corner, corner of lower index -> corner of higher index (one
 *               verdict per pair), query point -> source or corner.
 *   nodes       the corners (x0,y0) (x1,y0) (x1,y1) (x0,y1) of every rectangle, in rectangle order, without those that lie
 *               strictly inside some rectangle.  Edge weight w(a, b) = sqrt(dx*dx + dy*dy).
 *   field       the least dist with  dist[c] = min(min over the sources s that see c of w(s, c),
 *                                                  min over the corners u that see c of fl(dist[u] + w(u, c))),
 *               inf where nothing reaches (what Dijkstra from the sources returns with the same additions).
 *   query       d(p) = min(min over the sources p sees of w(p, s), min over the corners p sees of fl(w(p, c) + dist[c])),
 *               inf when nothing is reachable (every segment out of a point strictly inside a rectangle is blocked).
 * Two rectangles that exactly abut leave a slit of zero width that a path may use: d can only come out shorter for it.
 *
 * vlfm_geodesic_fields: the fields of n environments, ONE launch (one workgroup per environment) on `stream`.
 *   d_world_boxes, d_box_counts, n_worlds, max_boxes, d_world_of [n]: the world table above and the world of each field
 *   margin          the inflation
 *   d_objects       [n][8][8] doubles: vlfm_worlds_raycast's records (x0 y0 x1 y1 z0 z1 valid pad)
 *   d_sources       [n][max_sources][2] doubles, d_source_counts [n] int32 (clamped to [0, max_sources]; 0: every dist is inf)
 *   d_rects         [n][R][4] doubles out, R = max_boxes + 8 whatever the counts;  d_nodes [n][4R][2] doubles out;
 *                   d_dist [n][4R] doubles out;  d_counts [n][2] int32 out: rectangles, nodes.  Table tails are zeros at
 *                   infinite distance.
 * The tables of 4R candidate nodes and their 4R x 4R visibility bitmap must fit 64 KB of LDS (VLFM_ERR_INVALID otherwise,
 * nothing launched): R <= 141.
 *
 * vlfm_geodesic_query: d of m points, ONE launch (one workgroup per point) on `stream`.
 *   d_points        [m][2] doubles;  d_field_of [m] int32: the field of each point; outside [0, n_fields): the answer is NaN
 *   d_rects, d_nodes, d_dist, d_counts, d_sources, d_source_counts, max_sources: the n_fields fields as built above;
 *                   n_boxes = the max_boxes they were built with
 *   d_out           [m] doubles
 * n == 0 and m == 0 return VLFM_OK without a launch. */
int vlfm_geodesic_fields(const double* d_world_boxes, const int32_t* d_box_counts, int n_worlds, int max_boxes,
                         const int32_t* d_world_of, double margin, const double* d_objects, const double* d_sources,
                         const int32_t* d_source_counts, int n, int max_sources, double* d_rects, double* d_nodes,
                         double* d_dist, int32_t* d_counts, void* stream);
int vlfm_geodesic_query(const double* d_points, const int32_t* d_field_of, int m, int n_fields, int n_boxes,
                        const double* d_rects, const double* d_nodes, const double* d_dist, const int32_t* d_counts,
                        const double* d_sources, const int32_t* d_source_counts, int max_sources, double* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Map planner (ABI 21, csrc/map_planner.hip): shortest paths over the navigable planes of the obstacle maps (the reference's
 * _navigable_map: obstacles dilated by the robot's footprint, unexplored cells free), n jobs in ONE launch, one workgroup per
 * job.  Integers only; bit for bit vlfm_amd.synthetic.plan_paths_numpy (Dijkstra with a heap over the same rule).
 *
 * A JOB plans one path in one environment's plane.  Cells are (x, y) = (bit, row) of the bit-packed plane (row = ceil(size / 32)
 * 32-bit words, bit x of a row in word x >> 5 at position x & 31); metres become cells by BaseMap._xy_to_px.
 *   env          the slot.  Two jobs may name the same slot.
 *   window       y0, y1, x0, x1, inclusive.  Everything outside it is blocked.
 *   start        (sx, sy) with a free radius start_free, in cells;  goal: (gx, gy) with goal_free.  Radii in [0, 4096].
 *   free         a cell of the window is free if its navigable bit is set, or if dx*dx + dy*dy <= r*r (integers) about `start`
 *                with r = start_free, or about `goal` with r = goal_free (r = 0: the cell itself -- start and goal are always
 *                free).  The discs exist because a robot legally stands inside the inflated zone next to a wall, and an object
 *                goal lies inside its own obstacle.
 *   moves        8-connected; cost 2 for E/N/W/S, 3 for diagonals.  a -> b is allowed iff both cells are free; a diagonal move
 *                also needs the two cells that share an edge with both a and b to be free (no corner cutting, no squeezing
 *                through a diagonal gap).  The rule is symmetric: a field grown from the goal is the distance TO the goal.
 *   field        dist[c] = the least cost from `goal` to c, uint16; 0xFFFF: blocked, outside the window, not reached, or cost
 *                above max_cost (an argument: at most 65534).
 *   descent      cur = start; while dist[cur] > 0 and fewer than `lookahead` steps were taken: try the chain codes s = 0..7
 *                (dx = {1,1,0,-1,-1,-1,0,1}, dy = {0,-1,-1,-1,0,1,1,1}: E NE N NW W SW S SE, y grows downwards) and take the
 *                first whose move is allowed and has dist[next] + cost(s) == dist[cur] (one always exists).  The waypoint is
 *                the final cur, `steps` the number of moves taken.
 *   result       status, cost, waypoint_x, waypoint_y, steps.  The status is the first that applies:
 *                  VLFM_PLAN_INVALID      env outside [0, n_envs), empty window, window outside the map or larger than
 *                                         field_h x field_w, start or goal outside the window, a radius outside [0, 4096].
 *                                         Nothing else is computed; a bad job never faults.
 *                  VLFM_PLAN_TOO_LONG     start has no cost <= max_cost and some cell has a finite cost above max_cost
 *                                         (the search reached max_cost with cells still to expand)
 *                  VLFM_PLAN_UNREACHABLE  the search ran dry without reaching start
 *                  VLFM_PLAN_OK           cost = dist[start], waypoint and steps as above
 *                Every status but VLFM_PLAN_OK: cost = 0xFFFF, waypoint = start, steps = 0.
 * cost * 0.5 / pixels_per_meter is the path length in metres; it overstates pure diagonals by 6 % (3/2 against sqrt 2).
 *
 * vlfm_plan_paths, on `stream` (a memset node presets the dist planes, then ONE kernel):
 *   d_navigable   [n_envs][size][ceil(size / 32)] words, size <= 2048
 *   d_jobs        [n_jobs] VlfmPlanJob;  d_results [n_jobs] VlfmPlanResult out
 *   lookahead     >= 0, steps of the descent;  max_cost in [0, 65534]
 *   d_fields      NULL, or [n_jobs][field_h][field_w] uint16 out: row / column 0 are the window's y0 / x0, cells beyond the
 *                 window (and the whole field of an invalid job) are 0xFFFF.  NULL: no field is kept and the search stops
 *                 after the level that settles `start` (every cell of a shortest path from it is settled by then): the
 *                 results are those of the full run.
 *   field_h, field_w   in [1, size]: the bound every job's window keeps to, with or without d_fields (the dist planes and the
 *                 LDS planes are laid out for it).  The jobs are device memory, which the host call cannot inspect, so a
 *                 window beyond the bound is answered per job (VLFM_PLAN_INVALID); the Python layer derives the bound from
 *                 the jobs it uploads.
 *   d_scratch     at least vlfm_plan_scratch_bytes(n_jobs, size) bytes (VLFM_ERR_CAPACITY otherwise); no state between calls
 * Returns VLFM_PLAN_IN_LDS (0) when the six bit planes of a field_h x field_w window fit 160 KB of LDS (e.g. 400 x 400), else
 * VLFM_PLAN_IN_SCRATCH (1): they then live in d_scratch.  Same results either way.  Negative: vlfm_status, nothing launched.
 * n_jobs == 0 returns 0 without a launch. */
enum { VLFM_PLAN_OK = 0, VLFM_PLAN_UNREACHABLE = 1, VLFM_PLAN_TOO_LONG = 2, VLFM_PLAN_INVALID = 3 };
enum { VLFM_PLAN_IN_LDS = 0, VLFM_PLAN_IN_SCRATCH = 1 };
typedef struct VlfmPlanJob {
    int32_t env, y0, y1, x0, x1;
    int32_t sx, sy, start_free;
    int32_t gx, gy, goal_free;
    int32_t reserved;
} VlfmPlanJob; /* 48 bytes */
typedef struct VlfmPlanResult {
    int32_t status, cost, waypoint_x, waypoint_y, steps;
    int32_t reserved[3];
} VlfmPlanResult; /* 32 bytes */
size_t vlfm_plan_scratch_bytes(int n_jobs, int size);
int vlfm_plan_paths(const int32_t* d_navigable, int n_envs, int size, const VlfmPlanJob* d_jobs, int n_jobs, int lookahead,
                    int max_cost, uint16_t* d_fields, int field_h, int field_w, VlfmPlanResult* d_results, void* d_scratch,
                    size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Lattice geodesic (ABI 26, csrc/lattice_geodesic.hip): the ObjectNav metrics' geodesic for worlds the visibility graph above
 * cannot hold -- grid worlds, box worlds beyond 141 rectangles -- on a metric lattice with integer costs.  Bit for bit
 * vlfm_amd.synthetic.lattice_free_numpy / lattice_field_numpy / lattice_query_numpy; integers everywhere except the free test
 * and the query (f64, one rounding per operation, no fused multiply-add).
 *   lattice     n = cells_per_metre, a multiple of 4.  Node (a, b), global integers, sits at (a / n, b / n), true divisions.
 *               Field f covers a0 .. a0 + na - 1 by b0 .. b0 + nb - 1: d_dims [n][4] int32 = a0, b0, na, nb, with na and nb
 *               clamped to [0, max_na] and [0, max_nb] by the kernels (a zero: the field has no nodes).  Nodes outside do not
 *               exist.  max_nb and max_na, in [1, VLFM_LATTICE_MAX_NODES], are the strides of every plane of a call.
 *   free        node (x, y) is blocked iff some obstacle has x0 - m < x < x1 + m and y0 - m < y < y1 + m (OPEN sets, the
 *               expressions of the geodesic above): the `count` boxes of the field's world, the occupied cells of its grid, the
 *               object slots with valid != 0.  Grid cells are not looped over: edge - m and edge + m are monotone in the edge,
 *               two strict binary searches per axis give the block of cells that pass, and the node is blocked iff a bit of
 *               that block is set.  Free planes: uint32 [n][max_nb][ceil(max_na / 32)], bit a % 32 of word a / 32 of row b
 *               (local indices); vlfm_lattice_free writes zeros beyond a field's dims.
 *   moves       16-connected: cost 5 straight, 7 diagonal, 11 for a knight move (+-2, +-1) / (+-1, +-2).  Both ends free, and
 *               the intermediate nodes: a diagonal needs the two nodes that share an edge with both ends; a knight move (2s, t)
 *               from (a, b) needs (a + s, b) and (a + s, b + t); (s, 2t) needs (a, b + t) and (a + s, b + t).  Symmetric.
 *   sources     d_sources [n][max_sources][2] int32 global nodes (a, b), d_source_counts [n] (clamped to [0, max_sources]);
 *               a source outside its lattice or on a blocked node is ignored.
 *   field       d_dist uint16 [n][max_nb][max_na]: the least cost over move sequences from a source; 0xFFFF: none, above
 *               max_cost (in [0, 65534]), or beyond the field's dims.
 *   query       p = (x, y) in field f: fa = floor(x * n), fb = floor(y * n); over the four nodes (fa | fa + 1, fb | fb + 1)
 *               that lie in the lattice and hold a cost, d = min fl(sqrt(dx*dx + dy*dy) + cost / (5.0 * n)) with
 *               dx = x - a / n, dy = y - b / n; inf if none qualifies; a field outside [0, n_fields): NaN.
 * cost / (5 n) is the path length in metres; in free space it lies within [0.98387, 1.01980] of the Euclidean length.
 *
 * vlfm_lattice_free: the free planes of n fields (n <= 65535), ONE launch on `stream`.  World table, grids (all three arrays
 * or all three NULL), d_world_of, margin and d_objects (NULL: no objects) as in vlfm_worlds_raycast_grids / vlfm_geodesic_fields.
 * vlfm_lattice_fields: a memset that presets d_dist, then ONE kernel, one workgroup per field.  It reads free planes, never
 * worlds; whatever the planes hold beyond a field's dims is ignored.  Returns VLFM_LATTICE_IN_LDS (0) when the fourteen bit
 * planes of a max_nb x max_na lattice fit 160 KB of LDS (e.g. 256 x 256); else VLFM_LATTICE_IN_SCRATCH (1): `free` and `open`
 * stay in LDS and the twelve level planes live in d_scratch (while two planes fit: up to about 780 x 780); else
 * VLFM_LATTICE_ALL_IN_SCRATCH (2).  d_scratch: at least vlfm_lattice_scratch_bytes(n, max_nb, max_na) bytes (0 when LDS holds
 * everything; VLFM_ERR_CAPACITY if the scratch is smaller).  Same results in all three.
 * vlfm_lattice_query: d of m points, ONE launch.
 * A bound outside [1, 1024], cells_per_metre not a positive multiple of 4, negative counts, max_cost outside [0, 65534] or a
 * missing array: VLFM_ERR_INVALID, nothing launched, nothing written.  n == 0 and m == 0 return VLFM_OK without a launch. */
#define VLFM_LATTICE_MAX_NODES 1024
enum { VLFM_LATTICE_IN_LDS = 0, VLFM_LATTICE_IN_SCRATCH = 1, VLFM_LATTICE_ALL_IN_SCRATCH = 2 };
int vlfm_lattice_free(const double* d_world_boxes, const int32_t* d_box_counts, int n_worlds, int max_boxes,
                      const uint32_t* d_grid_bits, const double* d_grid_edges, const int32_t* d_grid_dims, int max_nx, int max_ny,
                      const int32_t* d_world_of, double margin, const double* d_objects, const int32_t* d_dims, int n,
                      int cells_per_metre, int max_nb, int max_na, uint32_t* d_free, void* stream);
size_t vlfm_lattice_scratch_bytes(int n, int max_nb, int max_na);
int vlfm_lattice_fields(const uint32_t* d_free, const int32_t* d_dims, int n, int max_nb, int max_na, const int32_t* d_sources,
                        const int32_t* d_source_counts, int max_sources, int max_cost, uint16_t* d_dist, void* d_scratch,
                        size_t scratch_bytes, void* stream);
int vlfm_lattice_query(const double* d_points, const int32_t* d_field_of, int m, int n_fields, const uint16_t* d_dist,
                       const int32_t* d_dims, int max_nb, int max_na, int cells_per_metre, double* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth sensor (ABI 27, csrc/depth_sensor.hip): what a depth camera makes of the exact frames vlfm_worlds_raycast writes --
 * axial noise, disparity quantisation, holes -- for n frames in ONE launch on `stream`, bit for bit
 * vlfm_amd.synthetic.depth_sensor_numpy (f32, one rounding per operation, no fused multiply-add).  Per frame i, with
 * kf = d_keys[i] (synthetic.DepthSensor.frame_keys: the hash of seed, environment and clock, made on the host),
 * lo = d_range[i][0], hi = d_range[i][1], span = hi - lo, p = r * W + u, mix32 the mixer of world_render.hip:
 *   metres    z = lo + d * span
 *   invalid   any of: min_range_m > 0 or max_range_m < inf, and not (z >= min_range_m and z <= max_range_m);
 *             edge_m > 0 and |z_n - z| > edge_m for a neighbour above, below, left or right inside the frame;
 *             mix32(kf, p, 55) < drop_threshold;  mix32(kf, (r >> 3) * ((W + 7) >> 3) + (u >> 3), 56) < patch_threshold
 *             (a threshold of 0: the stage is off).  An invalid pixel is written as 0.0f.
 *   noise     (sigma0_m or sigma2_per_m not 0)  h1 = mix32(kf, p, 53), h2 = mix32(kf, p, 54),
 *             nf = f32((h1 & 0xFFFF) + (h1 >> 16) + (h2 & 0xFFFF) + (h2 >> 16) - 131070) * f32(1 / sqrt(1431655765)),
 *             z1 = z + (sigma0_m + sigma2_per_m * (z * z)) * nf
 *   quantise  (disparity_k > 0)  z1 = z1 < 1e-3f ? 1e-3f : z1;  m = rint(k / z1);  m = m < 1 ? 1 : m;  z1 = k / m
 *   output    v = (z1 - lo) / span;  v < 1e-3f ? 1e-3f : (v > 1 ? 1 : v)
 *   With noise and quantisation both off a valid pixel is the input value, bit for bit (nothing is computed for it).
 * d_clean, d_out: f32 [n][H][W]; they must not overlap (the edge stage reads clean neighbours).  d_keys uint32 [n], d_range
 * f32 [n][2].  d_invalid: NULL, or int32 [n] that receives the invalid pixels of each frame (zeroed by a memset on `stream`
 * first).  band_rows: rows per workgroup, 0: planned by the library (the ray caster's plan, rounded up to whole 8-row blocks).
 * With W % 4 == 0 and both planes 16-byte aligned a lane moves its four columns with one 16-byte load and one 16-byte store;
 * any other width or alignment takes scalar loads and stores.
 * NULL planes (or keys, ranges) with n > 0, n < 0 or n > 65535, H < 1, W < 1, H * W >= 2^31, band_rows < 0, a negative or NaN
 * scalar, or overlapping planes: VLFM_ERR_INVALID, nothing launched, nothing written.  n == 0: VLFM_OK without a launch. */
int vlfm_depth_sensor(const float* d_clean, float* d_out, int n, int H, int W, const uint32_t* d_keys, const float* d_range,
                      float sigma0_m, float sigma2_per_m, float disparity_k, uint32_t drop_threshold, uint32_t patch_threshold,
                      float edge_m, float min_range_m, float max_range_m, int32_t* d_invalid, int band_rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth filter (ABI 28, csrc/depth_filter.hip): the holes of n depth frames (zeros, NaN, negatives) filled from the nearest valid
 * pixels of their row and column, in two launches on `stream` (a row pass, a column pass) and the memset of the counts; bit for
 * bit vlfm_amd.synthetic.depth_filter_numpy.  Values are only selected, never computed.  The rule is this project's own: it
 * follows the contract of depth_camera_filtering.filter_depth ("fills zero pixels from valid neighbours, optionally restores
 * originally non-zero pixels") and claims no arithmetic parity with that library, whose source is pinned nowhere.  Per pixel d:
 *   positive   d > 0 (NaN, +0.0, -0.0 and negatives are not)
 *   source     positive, and with clip_far > 0 not (d > clip_far): a value equal to clip_far stays a source
 *   kept       recover_nonzero ? positive : source.  A kept pixel leaves with its input bits; every other pixel is a hole
 *   candidate  per direction left, right, up, down: the value of the nearest source of d_in in that direction inside the frame,
 *              if reach_px == 0 or it is at most reach_px steps away.  Candidates are input pixels: a fill never feeds a fill
 *   hole       the maximum (fill == 0, "far") or minimum (fill == 1, "near") of its candidates; without one: set_black ?
 *              black_value : 0.0f
 * d_in, d_out: f32 [n][H][W]; they must not overlap.  d_counts: NULL, or int32 [n][2] that receives per frame the holes that had
 * a candidate and the holes that had none (zeroed by a memset on `stream` first).  band_rows: rows per workgroup of the column
 * pass, 0: planned by the library; the result is the same for every value.  With W % 4 == 0 and both planes 16-byte aligned a
 * lane moves its four columns 16 bytes at a time; any other width or alignment takes scalar loads and stores.
 * NULL planes with n > 0, n < 0 or n > 65535, H < 1, W < 1, H * W >= 2^31, band_rows < 0, fill not 0 or 1, reach_px outside
 * [0, 65535], a negative or non-finite clip_far, a non-finite black_value, or overlapping planes: VLFM_ERR_INVALID, nothing
 * launched, nothing written.  n == 0: VLFM_OK without a launch. */
int vlfm_depth_filter(const float* d_in, float* d_out, int n, int H, int W, int fill, int reach_px, float clip_far,
                      int recover_nonzero, int set_black, float black_value, int32_t* d_counts, int band_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLFM_AMD_H */
