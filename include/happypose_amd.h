/*
 * happypose_amd -- C ABI of the MI355X-native render-and-compare refinement path.
 *
 * This header is the drop-in boundary.  The reference is pure
 * Python with no FFI on this path, so each entry point replaces a Python-level
 * interface of the reference; the citation next to it is the reference function it
 * stands in for (paths relative to the reference root; TB/ = happypose/toolbox/,
 * MP/ = happypose/pose_estimators/megapose/, CP/ = happypose/pose_estimators/cosypose/cosypose/).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every `d_*` pointer is DEVICE memory (HBM), every
 *    `h_*` pointer is host memory; float = IEEE fp32; poses are row-major 4x4, intrinsics
 *    row-major 3x3.
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream) and returns without synchronising; no hidden allocations after create().
 *  - return value 0 = success, negative = error (hp_last_error() gives the text).  Shape
 *    or argument errors are reported, never silently repaired -- mirroring the reference's
 *    asserts (e.g. TB/renderer/panda3d_batch_renderer.py:166-169).
 *  - non-finite poses/intrinsics render as all-zero images, not an error
 *    (TB/renderer/panda3d_batch_renderer.py:81-111).
 */
#ifndef HAPPYPOSE_AMD_H
#define HAPPYPOSE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations of this header -- and nothing else -- are its dynamic
 * symbols (tests/test_abi.py: nm -D shows the hp_* entry points only). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define HP_OK 0
#define HP_ERR_ARG -1
#define HP_ERR_HIP -2
#define HP_ERR_STATE -3

int hp_version(void);
const char* hp_last_error(void);
/* number of visible HIP devices / name of the current one (diagnostics) */
int hp_device_count(void);
int hp_device_name(char* buf, int len);

/* ------------------------------------------------------------------------------------
 * Mesh store: device-resident geometry + textures of an object set, and the padded
 * mesh-point database.  Replaces Panda3dBatchRenderer.__init__(asset_dataset, ...)
 * (TB/renderer/panda3d_batch_renderer.py:129-142, worker start-up :288-330, model cache
 * TB/renderer/panda3d_scene_renderer.py:206-219) and MeshDataBase.batched().to(device)
 * (TB/lib3d/rigid_mesh_database.py:84-130).
 *
 * h_obj: [n_obj][8] int64 = vert_off, n_verts, face_off, n_faces, tex_off(-1 none),
 *        tex_w, tex_h, 0.   faces hold vertex ids LOCAL to their object.
 * h_points: [n_obj][n_pad][3] metres (may be NULL when only rendering is needed).
 * ---------------------------------------------------------------------------------- */
typedef struct hp_mesh_store hp_mesh_store;

hp_mesh_store* hp_mesh_store_create(const float* h_verts, const float* h_normals,
                                    const float* h_uvs, const uint8_t* h_colors,
                                    int64_t n_verts_total, const int32_t* h_faces,
                                    int64_t n_faces_total, const uint8_t* h_tex,
                                    int64_t tex_bytes, const int64_t* h_obj, int n_obj,
                                    const float* h_points, int n_pad);
void hp_mesh_store_destroy(hp_mesh_store* store);
/* device pointer of the [n_obj][n_pad][3] point table (NULL if not uploaded) */
const float* hp_mesh_store_points(const hp_mesh_store* store);
/* The rasteriser keeps per-(view, band) triangle lists and per-(view, vertex) records in scratch memory owned by the
 * store; it grows on demand (never under stream capture: hp_rasterize then fails with HP_ERR_ARG).  Reserve it for the
 * largest call -- n_views views of h x w, flags: HP_RASTER_MSAA4 if multisampled renders will be asked for -- so that no
 * later call reallocates it (the reference's worker pool pre-loads its scene the same way,
 * TB/renderer/panda3d_batch_renderer.py:129-142).  hp_mesh_store_scratch_generation counts the reallocations: a holder
 * of captured hipGraphs that launch hp_rasterize compares it before every replay. */
int hp_mesh_store_reserve_raster(hp_mesh_store* store, int n_views, int h, int w, int flags);
int64_t hp_mesh_store_scratch_generation(const hp_mesh_store* store);

/* ------------------------------------------------------------------------------------
 * Rasteriser.  Replaces Panda3dBatchRenderer.render(labels, TCO, K, light_datas,
 * resolution, render_normals, render_depth, render_binary_mask) -> BatchRenderOutput
 * (TB/renderer/panda3d_batch_renderer.py:194-286; worker :62-125; scene renderer
 * TB/renderer/panda3d_scene_renderer.py:320-390; camera model TB/renderer/types.py:92-137;
 * depth decode / normal code TB/renderer/utils.py:46-79).
 *
 * One mesh per view, pinhole camera K, pose TCO, clip range [0.1, 10] m, two-sided,
 * black background.  Outputs (each may be NULL = not rendered):
 *   rgb   3 ch f32 in [0,1]   albedo * (ambient + Lambert point lights), 8-bit quantised
 *   nrm   3 ch f32 in [0,1]   eye-space normal colour code
 *   depth 1 ch f32 metres, 0 = background (or normalised, see below)
 *   mask  u8 [n][h][w]        depth > 0   (requires depth, as the reference asserts)
 * Addressing of the float outputs (element strides), view = 0..n-1:
 *   off(view, c, row, col) = (view / views_per_item) * s_item + (view % views_per_item) * s_view
 *                            + c * s_chan + row * s_row + col * s_col
 * so both the reference's NCHW BatchRenderOutput tensors and channel slices of the
 * NHWC network input are expressible.  depth uses (ds_item, ds_view, ds_row, ds_col).
 * d_depth_norm_z (optional, [n / views_per_item]): fuses normalize_images
 * (MP/models/pose_rigid.py:455-544) into the epilogue; depth_norm_mode selects
 * 0 none, 1 tCR_scale (d/z), 2 tCR_scale_clamp_center (clamp(d/z,0,2)-1),
 * 3 tCR_center_clamp (clamp(d-z,-2,2)).
 * ---------------------------------------------------------------------------------- */
#define HP_RASTER_QUANT8 8
/* d_rgb / d_nrm / d_depth point at fp16 tensors (strides in fp16 elements): views rendered straight into
 * the input of an fp16 network plan (hp_net_forward_f16in).  The mask stays uint8. */
#define HP_RASTER_OUT_F16 16
/* 4x multisampled colour / normal buffers, the framebuffer state of the reference's renderer
 * (TB/renderer/panda3d_scene_renderer.py:70-71 "framebuffer-multisample 1 / multisamples 4"): coverage and depth per
 * sample (standard 4x pattern), one shading per pixel and triangle at the pixel centre, 8-bit resolve = mean of the four
 * samples.  Depth and mask stay sampled at the pixel centre.  Ignored by depth-only renders. */
#define HP_RASTER_MSAA4 32
/* Texture filtering of the reference's renderer (TB/renderer/panda3d_scene_renderer.py:68-69 "texture-minfilter mipmap",
 * "texture-anisotropic-degree 16"): trilinear over the mip chain the store keeps behind level 0 (obj row entry 7 = number
 * of levels) + up to 16 probes along the major axis of the pixel footprint (EXT_texture_filter_anisotropic's sketch).
 * Default (flag clear): bilinear on level 0. */
#define HP_RASTER_TEX_ANISO 64

typedef struct {
  int64_t s_item, s_view, s_chan, s_row, s_col;
} hp_strides;

/* The three conventions of the reference's renderer that OpenGL / Panda3D leave to the implementation and that cannot be
 * pinned without Panda3D: where the four multisample positions sit, how the anisotropic filter
 * derives its probe count and level of detail from the pixel footprint, and which eye-space axis (and sign) each
 * channel of the normal-code render shows (TB/renderer/panda3d_scene_renderer.py:68-71,221-230, TB/renderer/utils.py:63-79).
 * They are a RECORD, not compile-time constants, so that an owner of a Panda3D installation can fit them:
 * tools/calibrate_renderer.py scores candidate records against Panda3D renders of the reference's own test scene
 * (tests/test_batch_renderer_panda3d.py:43-69); oracle/csrc/oracle.c mirrors the record (hp_oracle_set_raster_conventions).
 * The record belongs to a MESH STORE (hp_mesh_store_set_raster_conventions; NULL restores the defaults below) and is read at
 * launch time: two stores -- two renderers -- in one process may differ; launches already enqueued keep the values they were
 * launched with; captured hipGraphs must be re-captured after a change.  Sample positions are used on a 1/256-pixel grid
 * (rounded to nearest; hardware keeps them on such a grid -- D3D: 1/16 --, and so does the oracle). */
typedef struct {
  float msaa_x[4], msaa_y[4];  /* sample positions inside the pixel, each in (0, 1).  Default: the standard 4x pattern
                                  (0.375, 0.125) (0.875, 0.375) (0.125, 0.625) (0.625, 0.875) */
  int aniso_max;               /* cap of the probe count, 1..16 ("texture-anisotropic-degree").  Default 16 */
  int aniso_round;             /* probes from the footprint ratio r = Pmax / Pmin: 0 ceil(r) (default, the extension's sketch),
                                  1 nearest integer (ties to even), 2 floor(r) */
  int lod_from;                /* level of detail = log2 of: 0 Pmax / N (default), 1 Pmin, 2 Pmax (no anisotropic compensation) */
  float lod_bias;              /* added to the level of detail before clamping.  Default 0 */
  float aniso_ratio_bias;      /* added to r before it is rounded to the probe count.  Default 0 */
  int normal_axis[3];          /* channel c of the normal-code render shows component normal_axis[c] of the unit normal in the
                                  CAMERA frame of this library (OpenCV: x right, y down, z forward) ... */
  float normal_sign[3];        /* ... times normal_sign[c] (+1 / -1).  Default axes {0, 1, 2}, signs {+1, -1, -1}: GL eye space
                                  (x right, y up, z backward) as R, G, B */
} hp_raster_conventions;
int hp_mesh_store_set_raster_conventions(hp_mesh_store* store, const hp_raster_conventions* conventions /* NULL = defaults */);
int hp_mesh_store_get_raster_conventions(const hp_mesh_store* store, hp_raster_conventions* out);
/* Back-face culling in the set-up pass of this store's renders (read at launch time; default on, HP_RASTER_NO_CULL=1 creates
 * stores with it off).  The reference renders two-sided (TB/renderer/panda3d_scene_renderer.py:102).  A triangle whose
 * inward side is turned to the camera is dropped only when it cannot be seen: it belongs to a CONNECTED COMPONENT of the
 * (position-welded) mesh that is a closed, consistently oriented surface with a non-zero signed volume -- decided per
 * component at hp_mesh_store_create, so nested shells, parts with flipped winding and open sheets each get their own
 * answer --, the camera is outside the object's bounding sphere and the sphere lies beyond the near plane.  The facing test
 * is the exact sign of the triangle's area on the 1/256-px vertex grid.  Pixels may differ from the two-sided render only
 * where a sample lies exactly on a silhouette edge.  ASSUMPTION: a closed component does not intersect itself.  The edge test
 * and the net signed volume cannot see a self-intersecting component with a lobe of the opposite winding: its visible faces
 * would be culled (holes in rgb / depth / mask where the reference, two-sided, has none).  For object sets that may hold such
 * meshes switch culling off on the store -- hp_mesh_store_set_backface_culling(store, 0) right after hp_mesh_store_create, or
 * HP_RASTER_NO_CULL=1 for every store of the process; renders are then two-sided everywhere, ~25 % slower.
 * Returns the previous setting (-1: null store). */
int hp_mesh_store_set_backface_culling(hp_mesh_store* store, int on);
/* The current setting (1 / 0; -1: null store): what a lane's store copies from the store it was cloned from. */
int hp_mesh_store_get_backface_culling(const hp_mesh_store* store);

int hp_rasterize(const hp_mesh_store* store, int n, int views_per_item,
                 const int32_t* d_obj_ids /* [n / views_per_item] */,
                 const float* d_TCO /* [n][16] */, const float* d_K /* [n][9] */,
                 const float* d_ambient /* [n][3] or NULL = (1,1,1) */, int n_lights,
                 const float* d_light_pos /* [n][n_lights][3] object frame */,
                 const float* d_light_col /* [n][n_lights][3] */, int h, int w, int flags,
                 float* d_rgb, float* d_nrm, const hp_strides* color_strides,
                 float* d_depth, const hp_strides* depth_strides, uint8_t* d_mask,
                 const float* d_depth_norm_z, int depth_norm_mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Network input of one refiner / scoring iteration in ONE pass: render the views of every hypothesis AND crop the
 * observation, each pixel record of the NHWC input written once.  Replaces, per iteration,
 *   crop_inputs -> crop_images (torchvision roi_align)       MP/models/pose_rigid.py:199-277, TB/lib3d/cropping.py:155-197
 *   render_images_multiview -> Panda3dBatchRenderer.render    MP/models/pose_rigid.py:376-453
 *   normalize_images + torch.cat((images_crop, renders))      MP/models/pose_rigid.py:455-544,624-629
 * (CosyPose: CP/models/pose.py:58-93,129-157).  Same arithmetic as hp_crop_roi_align followed by hp_rasterize into channel
 * slices; what changes is the memory traffic: no kernel touches a 32-B sector another kernel (or another workgroup) also
 * writes -- rocprofv3 counted 3x the algorithmic bytes for the two-launch form (profiles/r03a_raster_hbm_traffic.json).
 *
 * d_x: [n_items][h][w][record_elems] fp32, or fp16 with HP_RASTER_OUT_F16.  View v of an item writes
 *   its render channels -- rgb, then normals (HP_RENDER_NORMALS), then depth (HP_RENDER_DEPTH, normalised per
 *   depth_norm_mode as in hp_rasterize) -- at elements [view_c0[v], ...) of every pixel record, and
 *   crop_n[v] channels of the observed crop, source channels [crop_src0[v], crop_src0[v] + crop_n[v]) of the frame
 *   d_images[d_im_ids[item]] resampled from d_boxes[item] with torchvision's roi_align (sampling_ratio^2 samples,
 *   aligned = False; source channel 3 = depth: validity rule of TB/lib3d/cropping.py:184-195 and the same
 *   normalisation), at elements [crop_c0[v], ...).
 * The reference's channel order is {crop_n = {C_img, 0, ...}, crop_c0 = {0}, view_c0[v] = C_img + v * C_r}; any other
 * assignment (e.g. view v = one 32-B sector holding its 7 channels + crop channel v) needs the network's first layer
 * permuted accordingly.  Elements of a record nobody is assigned keep their value (the pads of a zeroed input stay 0).
 * ---------------------------------------------------------------------------------- */
#define HP_RENDER_NORMALS 0x1000
#define HP_RENDER_DEPTH 0x2000

typedef struct {
  int view_c0[8];   /* first record element of view v's render channels */
  int crop_c0[8];   /* first record element of the crop channels view v produces */
  int crop_src0[8]; /* first source channel of those */
  int crop_n[8];    /* how many (0 = this view produces no crop channel) */
} hp_input_layout;

int hp_render_inputs(const hp_mesh_store* store, int n_items, int views_per_item, const int32_t* d_obj_ids /* [n_items] */,
                     const float* d_TCV_O /* [n_items][V][16] */, const float* d_KV /* [n_items][V][9] */,
                     const float* d_ambient /* [n_items * V][3] or NULL */, int n_lights,
                     const float* d_light_pos /* [n_items * V][n_lights][3] */, const float* d_light_col, int h, int w,
                     int flags /* HP_RASTER_* | HP_RENDER_* */, const float* d_images /* [Bi][Ct][H][W] */, int Bi, int Ct,
                     int H, int W, const float* d_boxes /* [n_items][4] xyxy */, const int32_t* d_im_ids /* [n_items] */,
                     int sampling_ratio, const float* d_depth_norm_z /* [n_items] */, int depth_norm_mode, void* d_x,
                     int record_elems, const hp_input_layout* layout, void* stream);

/* ------------------------------------------------------------------------------------
 * Iteration prologue ("pose prep"), one launch for all hypotheses and views:
 *   [normalize_T]  TB/lib3d/transform_ops.py:107-120   (MP/models/pose_rigid.py:571)
 *   tCR            MP/models/pose_rigid.py:574-576     (tOR = 0 -> tCR = tCO)
 *   TCV_O          make_TCO_multiview, TB/lib3d/multiview.py:166-251 (:28-92)
 *   per view: project_points_robust -> boxes_from_uv -> deepim_boxes -> get_K_crop_resize
 *                  MP/models/pose_rigid.py:199-337 (crop_inputs, compute_crops_multiview),
 *                  CP/models/pose.py:58-93; TB/lib3d/camera_geometry.py:40-122;
 *                  TB/lib3d/cropping.py:27-75,113-152
 * View 0 uses n_points_main sub-sampled mesh points (2000), the extra views
 * n_points_extra (200); point ids are the deterministic RandomState(0) lists
 * (TB/lib3d/mesh_ops.py:74-84) computed once on the host.
 * multiview_type: 0 = single view (TCV_O = TCO), 1 = "TCO+front_1view",
 * 3 = "TCO+front_3views", 5 = "TCO+front_5views"; n_views must be 1 / 2 / 4 / 6.
 * Outputs: d_TCO_out [b][16] (normalised input pose), d_tCR [b][3], d_TCV_O [b][V][16],
 * d_boxes_rend [b][4], d_boxes_crop [b][4], d_K_crop [b][V][9] (view 0 = K_crop).
 * Index convention of the whole library: intrinsics and frames are tables [n_images] indexed by d_im_ids, never
 * per-hypothesis copies.  Ids live on the device, so they cannot be asserted here the way the reference's indexing
 * raises; a hypothesis whose image or object id lies outside its table reads row 0 and gets NaN outputs (NaN poses
 * render as zero images, an out-of-range image id crops to zeros) -- out-of-bounds memory is never touched.
 * ---------------------------------------------------------------------------------- */
int hp_pose_prep(const hp_mesh_store* store, int b, int n_views, int multiview_type,
                 int normalize, const float* d_TCO_in, const float* d_K /* [n_images][9] */, int n_images,
                 const int32_t* d_im_ids /* [b], values in [0, n_images) */, const int32_t* d_obj_ids /* [b] */,
                 const int32_t* d_point_ids_main, int n_points_main,
                 const int32_t* d_point_ids_extra, int n_points_extra, int im_h, int im_w,
                 int crop_h, int crop_w, float lamb, float* d_TCO_out, float* d_tCR,
                 float* d_TCV_O, float* d_boxes_rend, float* d_boxes_crop, float* d_K_crop,
                 void* stream);
/* The same with `remove_TCO_rendering` (TB/lib3d/multiview.py:189-236, MP/models/pose_rigid.py:609-611): the TCO view
 * itself is not rendered.  n_views counts the RENDERED views (multiview_type 3 -> 3, 5 -> 5; >= 2); d_TCV_O / d_K_crop hold
 * the look-at views only, each with the intrinsics of its own 200-point crop (compute_crops_multiview), and the K of the
 * observed crop (crop_inputs; what hp_pose_update needs) goes to d_K_crop_main [b][9].  remove_tco_rendering = 0 behaves
 * like hp_pose_prep (d_K_crop_main optional: a copy of view 0's K). */
int hp_pose_prep_views(const hp_mesh_store* store, int b, int n_views, int multiview_type, int remove_tco_rendering,
                       int normalize, const float* d_TCO_in, const float* d_K, int n_images,
                       const int32_t* d_im_ids, const int32_t* d_obj_ids,
                       const int32_t* d_point_ids_main, int n_points_main,
                       const int32_t* d_point_ids_extra, int n_points_extra, int im_h, int im_w,
                       int crop_h, int crop_w, float lamb, float* d_TCO_out, float* d_tCR,
                       float* d_TCV_O, float* d_boxes_rend, float* d_boxes_crop, float* d_K_crop,
                       float* d_K_crop_main, void* stream);

/* ------------------------------------------------------------------------------------
 * Crop.  Replaces crop_images / torchvision.ops.roi_align(images, [k,x1,y1,x2,y2],
 * (240,320), sampling_ratio=4, aligned=False)  (TB/lib3d/cropping.py:155-197,
 * CP/lib3d/cropping.py:129-134) incl. the RGB-D rule (depth zeroed where the roi-aligned
 * validity mask < 0.99) and, optionally, the depth normalisation of normalize_images.
 * d_images: [Bi][C][H][W] f32 (the reference's ObservationTensor layout); the first
 * n_channels (3 = rgb, 4 = rgbd) planes are cropped (a model without input_depth drops the
 * depth plane of an RGB-D observation, MP/models/pose_rigid.py:557-559).  Output
 * addressing as in hp_rasterize with views_per_item = 1 (s_view unused).
 * depth_norm_mode may carry HP_CROP_FULL_RECORD8: the destination is an NHWC tensor whose pixel records are
 * multiples of 32 B (8 floats / 16 halves; 32-B aligned) and the crop owns the first 32 B of each: its 3 / 4 channels AND zeros for the
 * rest of that 32-B sector are written as one full-sector store (the rasteriser writes its channels afterwards): a
 * partial-sector store costs the memory system a read-modify-write.
 * ---------------------------------------------------------------------------------- */
#define HP_CROP_FULL_RECORD8 0x100
int hp_crop_roi_align(const float* d_images, int Bi, int C, int n_channels, int H, int W,
                      const float* d_boxes /* [n][4] */, const int32_t* d_im_ids /* [n] */,
                      int n, int out_h, int out_w, int sampling_ratio, float* d_out,
                      const hp_strides* out_strides, const float* d_depth_norm_z,
                      int depth_norm_mode, void* stream);
/* The same with an fp16 destination (strides in fp16 elements): the crop of an fp16 network plan
 * (hp_net_set_precision) written straight into the tensor hp_net_forward_f16in reads. */
int hp_crop_roi_align_f16(const float* d_images, int Bi, int C, int n_channels, int H, int W,
                          const float* d_boxes, const int32_t* d_im_ids, int n, int out_h, int out_w,
                          int sampling_ratio, void* d_out_f16, const hp_strides* out_strides,
                          const float* d_depth_norm_z, int depth_norm_mode, void* stream);

/* ------------------------------------------------------------------------------------
 * Pose update.  Replaces PosePredictor.update_pose (MP/models/pose_rigid.py:339-350 ->
 * TB/lib3d/rotations.py:22-36 + TB/lib3d/cosypose_ops.py:34-62) and CosyPose's
 * apply_imagespace_predictions (CP/lib3d/cosypose_ops.py:18-42; d_tCR = NULL).
 * d_K_crop is [b][k_stride floats] (k_stride = 9 * n_views when taken from hp_pose_prep).
 * ---------------------------------------------------------------------------------- */
int hp_pose_update(int b, const float* d_TCO, const float* d_K_crop, int k_stride,
                   const float* d_pose9 /* [b][9] */, const float* d_tCR /* [b][3] or NULL */,
                   float* d_TCO_out, void* stream);

/* Coarse initialisation.  Replaces TCO_init_from_boxes_autodepth_with_R
 * (TB/lib3d/cosypose_ops.py:184-238; d_R != NULL), TCO_init_from_boxes_zup_autodepth
 * (:241-283; d_R = NULL).  Extents are taken over the full padded point set of the object
 * (MegaPose, MP/inference/pose_estimator.py:393-410) or, when d_point_ids is given, over
 * that deterministic sub-sample (CosyPose, CP/integrated/pose_estimator.py:128-130).
 * Hypothesis i uses box d_boxes[d_box_ids ? d_box_ids[i] : i], intrinsics
 * d_K[d_im_ids[i]], object d_obj_ids[i], rotation d_R[d_rot_ids ? d_rot_ids[i] : i]; an id outside its table
 * (sizes n_boxes / n_images / n_rots / objects of the store) gives a NaN pose, see hp_pose_prep. */
int hp_tco_init_autodepth(const hp_mesh_store* store, int n, const float* d_boxes /* [n_boxes][4] */, int n_boxes,
                          const int32_t* d_box_ids, const float* d_K /* [n_images][9] */, int n_images,
                          const int32_t* d_im_ids, const int32_t* d_obj_ids,
                          const float* d_R /* [n_rots][9] */, int n_rots, const int32_t* d_rot_ids,
                          const int32_t* d_point_ids, int n_points, float* d_TCO_out, void* stream);

/* ------------------------------------------------------------------------------------
 * Network (backbone + heads).  Replaces PosePredictor.net_forward
 * (MP/models/pose_rigid.py:352-374, CP/models/pose.py:108-114) for the backbones of
 * MP/training/pose_models_cfg.py:106-122 / CP/training/pose_models_cfg.py:39-42:
 *   HP_ARCH_VANILLA_RESNET34  MP/models/torchvision_resnet.py:191-344 (num_classes=512)
 *   HP_ARCH_WIDE_RESNET34/18  MP/models/wide_resnet.py:68-154 == CP/models/wide_resnet.py
 *   HP_ARCH_EFFICIENTNET_B3   CP/models/efficientnet.py:153-277 (extract_features; BN eps 1e-3,
 *                             static "same" padding for image_size 300), features [batch][1536]
 * Parameters are handed over by their reference state_dict names ("backbone.conv1.weight",
 * "backbone.layer1.0.bn1.running_var", "pose_fc.weight", "views_logits_head.bias", ...;
 * legacy names of TB/utils/models_compat.py are translated by the host side), fp32 host
 * arrays in PyTorch layout ([Cout][Cin][kh][kw]).  hp_net_finalize folds eval-mode
 * BatchNorm (eps 1e-5) and repacks to the kernels' layout.
 * Input: d_x NHWC [batch][h][w][c_pad], c_pad = hp_net_input_channels_padded(), pad
 * channels zero.  Outputs (each may be NULL): d_pose [batch][pose_dim],
 * d_logits [batch][n_logits], d_features [batch][512] (1536 for EfficientNet-b3).
 * ---------------------------------------------------------------------------------- */
#define HP_ARCH_VANILLA_RESNET34 0
#define HP_ARCH_WIDE_RESNET34 1
#define HP_ARCH_WIDE_RESNET18 2
#define HP_ARCH_EFFICIENTNET_B3 3 /* CP/models/efficientnet.py (CosyPose's released checkpoints): features [b,1536] */
/* ResNet-50 + FPN, the backbone of the Mask-RCNN detector (MP/models/mask_rcnn.py:22-42 -> torchvision
 * resnet_fpn_backbone("resnet50")); parameters by the names DetectorMaskRCNN registers ("backbone.body.layer1.0.conv1.weight",
 * "backbone.fpn.inner_blocks.0.0.weight", ...).  No heads: hp_net_forward(net, x, batch <= max_batch, NULL, NULL, NULL) fills
 * the five pyramid levels, read back with hp_net_feature_map. */
#define HP_ARCH_RESNET50_FPN 4

/* A feed-forward graph of convolutions the CALLER describes (the detector's RoI heads: fully connected layers are 7x7 /
 * 1x1 convolutions on [n][7][7][256], the mask head 3x3 convolutions on [n][14][14][256]).  hp_net_create(HP_ARCH_CUSTOM,
 * c_in, h, w), then hp_net_add_conv per layer in execution order (arena slots 0..31; in_slot -1 = the network input;
 * weight [cout][cin][k][k] and optional bias [cout] by parameter name; act 0 none / 1 ReLU; res_slot >= 0 adds that slot
 * before the activation), hp_net_add_output for every slot to read back, hp_net_set_param, hp_net_finalize, hp_net_forward
 * (heads NULL), hp_net_copy_feature_map.  Output channel counts are rounded up to 4 (zero rows).
 * The graph may also hold the ops of an EfficientNet MBConv block, or any prefix of one, which then run through the launches
 * the HP_ARCH_EFFICIENTNET_B3 plan picks for them (block-level tests):
 *   hp_net_add_conv with act 2 (swish): the 1x1 expansion; with HP_CONV_GATED or-ed into act: the 1x1 projection, whose input
 *     is multiplied by the gate of the hp_net_add_se before it (same slot, cin = its C);
 *   hp_net_add_dwconv: depthwise k x k (k 3 or 5, stride 1 or 2) + BatchNorm (eps 1e-3, folded) + swish on C % 4 == 0
 *     channels; weight [C][1][k][k] and the BatchNorm prefix ("<prefix>.weight / .bias / .running_mean / .running_var") by
 *     parameter name; pad = top / left padding, the bottom / right one follows from the explicit output size (Ho, Wo): the
 *     "same" padding of EfficientNet is asymmetric;
 *   hp_net_add_se: squeeze-excitation vector of slot in_slot [n][H][W][C]: mean over H x W -> "<prefix>._se_reduce" [Cse][C]
 *     + bias -> swish -> "<prefix>._se_expand" [C][Cse] + bias -> sigmoid (Cse <= 128). */
#define HP_ARCH_CUSTOM 5
#define HP_CONV_GATED 0x100

typedef struct hp_net hp_net;

hp_net* hp_net_create(int arch, int n_inputs, int h, int w);
void hp_net_destroy(hp_net* net);
int hp_net_add_conv(hp_net* net, const char* weight_name, const char* bias_name, int cin, int cout, int k, int stride, int pad,
                    int act, int H, int W, int in_slot, int out_slot, int res_slot);
int hp_net_add_dwconv(hp_net* net, const char* weight_name, const char* bn_prefix, int C, int k, int stride, int pad, int H, int W,
                      int Ho, int Wo, int in_slot, int out_slot);
int hp_net_add_se(hp_net* net, const char* prefix, int C, int Cse, int H, int W, int in_slot);
int hp_net_add_output(hp_net* net, int slot, int H, int W, int C);
int hp_net_input_channels_padded(const hp_net* net);
int hp_net_set_param(hp_net* net, const char* name, const float* h_data, int64_t numel);
/* The device-pointer sibling of hp_net_set_param for a FINALISED network: an asynchronous device-to-device copy on `stream`,
 * ordered like any launch, without a host round trip and without re-planning (head training: hp_adamw_step below).  Only the
 * tensors the head kernels read as plain fp32 can be replaced: "pose_fc.weight" / ".bias", "views_logits_head.weight" / ".bias"
 * and, on HP_ARCH_VANILLA_RESNET34, "backbone.fc.weight" / ".bias".  Every other name was folded or packed at finalise (conv and
 * BN weights) and is HP_ERR_ARG, as are a wrong element count and a head the network does not have.
 * hp_net_set_pooled_out: while d_pooled is not NULL every forward of a network with the fc also copies the fc's INPUT (the
 * spatial mean, [batch][512]) to d_pooled, on the forward's stream -- what hp_fc_backward reads; NULL switches it off again. */
int hp_net_set_param_device(hp_net* net, const char* name, const float* d_data, int64_t numel, void* stream);
/* ... and the way back: the same tensors copied out of the network (a trainer's master copy starts from them); same errors. */
int hp_net_get_param_device(hp_net* net, const char* name, float* d_data, int64_t numel, void* stream);
int hp_net_set_pooled_out(hp_net* net, float* d_pooled);
/* Arithmetic of the conv stack, to be chosen before hp_net_finalize:
 *   HP_PRECISION_F32 (default): fp32 MFMA, the reference's precision;
 *   HP_PRECISION_F16: weights / activations rounded to fp16 once per layer, fp32 accumulation
 *     (v_mfma_f32_32x32x16_f16) -- configuration C5 of SURVEY.md 8; the reference has no fp16
 *     path, the tolerance is stated in DESIGN.md.  hp_net_forward still takes / returns fp32. */
#define HP_PRECISION_F32 0
#define HP_PRECISION_F16 1
int hp_net_set_precision(hp_net* net, int precision);
int hp_net_precision(const hp_net* net);
int hp_net_finalize(hp_net* net, int max_batch);
/* Widths of the three outputs of a finalized network: pose_dim / n_logits are 0 when the checkpoint has no such head (what
 * PosePredictor.net_forward returns, MP/models/pose_rigid.py:352-374); the compiled operator library sizes its outputs with it. */
int hp_net_output_dims(const hp_net* net, int* pose_dim, int* n_logits, int* n_features);
/* The planned input map of a network: hp_net_forward strides its input by h * w * c_pad floats per sample (c_pad = channels
 * rounded up to 4; the fp16 plan's record width is hp_net_input_channels_f16), so a caller -- the compiled operator library's
 * net_forward and its Meta kernel -- checks a tensor's height and width against these before handing over the pointer
 * (the reference's backbone takes any H x W, MP/models/pose_rigid.py:352-374; a plan is built for one).  device = the HIP
 * device that was current in hp_net_create (weights and arena live there). */
int hp_net_input_dims(const hp_net* net, int* h, int* w, int* c_pad, int* device);
int hp_net_forward(hp_net* net, const float* d_x, int batch, float* d_pose, float* d_logits,
                   float* d_features, void* stream);
/* Feature-pyramid networks (HP_ARCH_RESNET50_FPN): number of output maps ('0', '1', '2', '3', 'pool' of torchvision's
 * BackboneWithFPN) and the map itself -- NHWC [batch][h][w][c] fp32 in the network's arena, valid until the next forward. */
int hp_net_n_feature_maps(const hp_net* net);
int hp_net_feature_map(const hp_net* net, int index, const float** d_ptr, int* h, int* w, int* c);
/* ... or copied (device to device, asynchronously on `stream`) into caller-owned memory [batch][h][w][c].  For
 * HP_ARCH_RESNET50_FPN maps 0..4 are the pyramid levels, 5..9 the RPN objectness logits of those levels ([h][w][4], 3 anchors
 * + one padding channel) and 10..14 the RPN box deltas ([h][w][12]) (torchvision models/detection/rpn.py: RPNHead, keys
 * "rpn.head.conv.0.0.*", "rpn.head.cls_logits.*", "rpn.head.bbox_pred.*"). */
int hp_net_copy_feature_map(const hp_net* net, int index, int batch, float* d_dst, void* stream);
/* Layer-level tests: the op list of a finalized network of any architecture, and taps on it.  The arena of a built-in plan
 * rotates a few slots, so an intermediate map is gone after a forward; a tap keeps it.
 *   hp_net_n_ops / hp_net_op_info: the ops in execution order.  kind HP_OP_*; name = the weight name of a convolution
 *     ("backbone.layer2.0.conv1.weight") or depthwise layer, the prefix of a squeeze-excitation, "" otherwise; k, stride, pad,
 *     act (HP_ACT values: 0 none, 1 ReLU, 2 swish); H, W, Cin the input map (Cin = the module's channel count), Ho, Wo, Cout the
 *     output map as stored, NHWC [Ho][Wo][Cout]; prologue = 1 when BatchNorm + ReLU is applied to the input; in_slot / res_slot /
 *     out_slot the arena slots read and written (-1 = the network input / none); elem_bytes 4 (fp32 plan) or 2 (fp16 plan).
 *     A squeeze-excitation reports H = positions pooled, W = 1, Cout = its reduced width; the head has no output map.
 *     path / materialised describe the LAST hp_net_forward: path = HP_PATH_* the launch that produced the op's output
 *     (HP_PATH_NONE before the first forward, HP_PATH_MIXED when the chunks of a batch > max_batch took different launches);
 *     materialised = 0 when no launch wrote the op's output map (a stem under pool fusion, an expansion under the MBConv
 *     front): known only at run time, it depends on algorithm, precision and guard state.
 *   hp_net_set_taps: d_dst[i] is caller-owned device memory [batch][Ho][Wo][Cout] x elem_bytes for op op_index[i];
 *     every forward copies the op's output there (device to device, on the launch stream) right after the launch that wrote
 *     it, all chunks of a batch > max_batch at their sample offsets; an op that is not materialised is not copied.  n = 0
 *     clears the taps.  Taps never change which kernels are launched or their arguments.  A forward with taps set on a
 *     stream that is capturing is refused (HP_ERR_ARG).  Taps are for tests; the predictors never set them. */
#define HP_OP_CONV 0
#define HP_OP_MAXPOOL 1
#define HP_OP_HEAD 2
#define HP_OP_DWCONV 3
#define HP_OP_SE 4
#define HP_OP_RESIZE 5
#define HP_PATH_NONE 0
#define HP_PATH_SPLIT3X3 1          /* split-fp16 3x3 kernels (conv_split.hip / conv_pp.hip) */
#define HP_PATH_SPLIT3X3_SHORTCUT 2 /* ... carrying the block's 1x1 / stride-2 shortcut as extra work items */
#define HP_PATH_RODE 3              /* a shortcut written by the previous op's launch */
#define HP_PATH_WINOGRAD 4
#define HP_PATH_IGEMM_SPLIT 5
#define HP_PATH_PATCH 6
#define HP_PATH_GENERIC 7
#define HP_PATH_STEM7_POOL 8        /* 7x7 stem + ReLU + max-pool, fp32 operands as fp16 halves */
#define HP_PATH_STEM7_POOL_F16 9    /* the same on the fp16 plan */
#define HP_PATH_STEM_SPLIT_POOL 10  /* 5x5 run-mode stem + ReLU + max-pool */
#define HP_PATH_IGEMM_SPLIT_POOL 11 /* any other stem + ReLU + max-pool */
#define HP_PATH_MBCONV_FRONT 12     /* 1x1 expansion + depthwise + pooling sums */
#define HP_PATH_FUSED_AWAY 13       /* skipped: the previous op's fused launch wrote this op's output */
#define HP_PATH_CONV_F16 14
#define HP_PATH_MAXPOOL 15
#define HP_PATH_MAXPOOL_F16 16
#define HP_PATH_HEAD 17
#define HP_PATH_DWCONV 18
#define HP_PATH_SE 19
#define HP_PATH_RESIZE 20
#define HP_PATH_MIXED 21
typedef struct {
  int kind, k, stride, pad, act;
  int H, W, Cin, Ho, Wo, Cout;
  int prologue, in_slot, res_slot, out_slot, elem_bytes;
  int path, materialised;
  char name[128];
} hp_op_info;
int hp_net_n_ops(const hp_net* net);
int hp_net_op_info(const hp_net* net, int index, hp_op_info* info);
int hp_net_set_taps(hp_net* net, int n, const int* op_index, void* const* d_dst);
/* GeneralizedRCNNTransform.normalize of the detector (torchvision models/detection/transform.py: (image - mean) / std per
 * channel; MaskRCNN defaults mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225)) fused with the layout change the conv
 * stack wants: d_images NCHW [n][3][h][w] in [0,1] (ObservationTensor.images[:, :3]) -> d_x NHWC [n][h][w][4], pad channel 0. */
int hp_detector_preprocess(const float* d_images, int n, int h, int w, const float* h_mean3, const float* h_std3,
                           float* d_x_nhwc4, void* stream);
/* The same with GeneralizedRCNNTransform.resize + batch_images in front (torchvision models/detection/transform.py:
 * _resize_image_and_masks = F.interpolate(bilinear, align_corners=False, recompute_scale_factor=True); batch_images pads
 * to a multiple of 32 with zeros): images [n,3,h_in,w_in] -> resized to [h_out,w_out], normalised, written into the
 * top-left of the zeroed canvas [n,h_pad,w_pad,4].  The caller computes the sizes (happypose_amd/detector.py). */
int hp_detector_preprocess_resize(const float* d_images, int n, int h_in, int w_in, int h_out, int w_out, int h_pad, int w_pad,
                                  const float* h_mean3, const float* h_std3, float* d_x_nhwc4, void* stream);
/* fp16 plan only: the input already in fp16, NHWC [batch][h][w][hp_net_input_channels_f16()] with the
 * channels past n_inputs zero (hp_crop_roi_align_f16 / hp_rasterize with HP_RASTER_OUT_F16 write it):
 * saves the fp32 -> fp16 conversion pass of hp_net_forward (5 % of a coarse-scoring step). */
int hp_net_input_channels_f16(const hp_net* net);
int hp_net_forward_f16in(hp_net* net, const void* d_x16, int batch, float* d_pose, float* d_logits,
                         float* d_features, void* stream);
/* total multiply-accumulate FLOPs (2*MAC) of one sample through conv + linear layers */
double hp_net_flops_per_sample(const hp_net* net);
/* Profiling of the dominant kernel: with hp_net_set_profiling(net, 1) every conv launch is
 * bracketed by a pair of HIP events recorded on the launch stream (no synchronisation).
 * hp_net_profile_collect waits for the recorded pairs and returns the summed kernel time
 * (ms), the number of launches, their ALGORITHMIC FLOPs (2 x M x Cout x kh x kw x Cin of the
 * direct convolution) and the FLOPs the matrix cores actually executed (less for the Winograd
 * layers, more where tiles / K are padded; in fp32-MFMA equivalents: an fp16 MFMA FLOP of the
 * split-fp16 layers counts 1/16, its share of matrix-pipe time) since the previous collect. */
int hp_net_set_profiling(hp_net* net, int enabled);
/* Parity tests / layer-level users: the kernel family hp_conv2d_nhwc / hp_conv2d_nhwc_f16 -- the SINGLE-LAYER entry points, which
 * have no network to carry a choice -- pick from.  Networks never read it (no process-wide state on a network's launch path:
 * hp_net_set_conv_algo below).  AUTO = for 3x3 layers the split-fp16 kernels (fp32 operands as two fp16 halves, three fp16 MFMAs
 * per product, fp32 accumulation: fp32-level accuracy while |activations| < 65504), else Winograd F(2x2,3x3), else the
 * patch-staged direct kernel, else the generic implicit GEMM; WINOGRAD = exact-fp32 arithmetic only; DIRECT = no Winograd either;
 * IGEMM = generic kernel only. */
#define HP_CONV_ALGO_AUTO 0
#define HP_CONV_ALGO_DIRECT 1
#define HP_CONV_ALGO_IGEMM 2
#define HP_CONV_ALGO_WINOGRAD_1WAVE 3 /* WINOGRAD, but the one-wave-per-SIMD schedule of the Winograd kernel */
#define HP_CONV_ALGO_WINOGRAD 4 /* exact-fp32 kernels only: Winograd, else patch-staged, else generic */
#define HP_CONV_ALGO_SPLIT 5 /* split-fp16 kernels (3 fp16 MFMAs per fp32 product) wherever they apply */
int hp_conv_select_algo(int algo);
/* The choice of ONE network (what the predictors and bench.py's exact-fp32 pass use; networks on different host threads /
 * streams do not interfere); algo = -1 returns the network to AUTO. */
int hp_net_set_conv_algo(hp_net* net, int algo);
/* The conv kernels cut the tiles of a partially filled last round along K so that one launch fills the GPU.  When
 * independent launches share the GPU (the two half-batch lanes of a predictor on two streams) the other stream fills
 * those CUs and the slicing only costs its reduction: 0 switches it off for this network, 1 back on (the default). */
int hp_net_set_tail_split(hp_net* net, int enabled);
/* Dynamic activation scale of the split-fp16 kernels (default on).  x = x_hi + x_lo in fp16 has an ABSOLUTE floor of 2^-25:
 * activations below ~0.1 lose relative bits (x_lo falls into the fp16 subnormals).  With the scale on, every launch tracks
 * max|y| of what it stores (one atomicMax per wave into a per-layer word) and a split-fp16 consumer multiplies what it
 * splits by the power of two that puts its input's bound at 2^13 -- exact, undone in the epilogue together with the
 * weights' scale; a layer whose activations sit at 1e-4 then keeps the 22 significant bits of the scheme, and the fp16
 * range cannot be left by a finite input.  0 restores the unscaled arithmetic (A/B, tests). */
int hp_net_set_act_scale(hp_net* net, int enabled);
/* Numerical guard of the default (split-fp16) kernels.  They carry fp32 activations through the fp16 matrix path as
 * hi/lo halves, which needs |activation| < 65504; beyond that a half becomes inf and the layer's output inf / NaN where
 * the reference's fp32 arithmetic stays finite.  Every split-fp16 launch reports a non-finite output to a host-visible
 * word of its network.  hp_net_status synchronises `stream`, returns the flags and clears HP_STATUS_NONFINITE:
 *   HP_STATUS_NONFINITE  a forward since the last call produced a non-finite value: ITS OUTPUTS ARE INVALID;
 *   HP_STATUS_EXACT_ONLY the network has switched to the exact-fp32 kernels (Winograd / direct; sticky): re-running
 *                        the same inputs now gives the reference's arithmetic.
 * hp_net_forward also reads the word (without synchronising) on entry, so once a completed forward has tripped the
 * guard every later forward runs on the exact kernels by itself.
 * HP_PRECISION_F16 networks are covered too: every fp16 launch that writes activations (stems, 1x1, 3x3, stride 2) sets
 * HP_STATUS_NONFINITE when a value it stores was inf / NaN in fp32 BEFORE the activation (ReLU would hide a NaN) or is
 * non-finite as the half it was rounded to; hp_net_status returns and clears it as above.  An fp16 network has no exact
 * kernels of its own: it never reports HP_STATUS_EXACT_ONLY, does not latch, and hp_net_force_exact is accepted without
 * effect.  The remedy is the caller's: run the stage again on an HP_PRECISION_F32 network of the same parameters (the
 * Python layer, happypose_amd.ops.Net, keeps such a sibling and does this by itself). */
#define HP_STATUS_NONFINITE 1
#define HP_STATUS_EXACT_ONLY 2
int hp_net_status(hp_net* net, void* stream, int* flags);
/* Sets (1) or clears (0) the sticky exact-fp32 state the guard enters by itself.  Multi-rank callers use it to keep the
 * ranks uniform: when ANY rank's guard fired, every rank forces its networks exact before the stage is repeated, so that
 * the merged rows come from one arithmetic and no rank is left alone on the slower kernels (pose_estimator.py::_guarded;
 * no counterpart in the reference, whose ranks all run ATen's fp32 convolutions).  0 returns to the default kernels. */
int hp_net_force_exact(hp_net* net, int enabled);
/* diagnostics: workgroups per CU the runtime grants conv tile variant 0 (128x128) / 1 (128x64) */
int hp_conv_occupancy(int variant);
/* hipGraph safety: launches so far, in this process, of kernels whose code object uses scratch (private segment > 0:
 * register spills of a rarely used tile variant; counted on the host at launch time, so also while a stream captures,
 * never during a replay).  A captured graph that contains such a launch replays wrongly on this runtime; the host layer
 * (happypose_amd/pose_predictor.py::_run_refine, no counterpart in the reference) compares the count around a predictor's
 * eager call and keeps that predictor on eager launches when it moved.  Stays 0 on the benchmarked configurations. */
long long hp_scratch_launches(void);
int hp_net_profile_collect(hp_net* net, double* conv_ms, int64_t* n_launches, double* conv_flops,
                           double* mfma_flops);
/* Several networks on several streams (the two half-batch lanes of a predictor run concurrently, so their summed
 * kernel time exceeds the wall time): hp_profile_mark_reference records a process-wide reference event on `stream`;
 * hp_net_profile_intervals returns the number of timed stretches pending for `net` and writes the start / end of the
 * first `cap` of them in ms after the reference (call it BEFORE hp_net_profile_collect, which releases them).  The
 * caller takes the union over the networks: the time during which any conv kernel was running. */
int hp_profile_mark_reference(void* stream);
int hp_net_profile_intervals(hp_net* net, double* t0_ms, double* t1_ms, int cap);

/* Diagnostics: the fp16 matrix-pipe rate this GPU SUSTAINS (back-to-back v_mfma_f32_32x32x16_f16 on every SIMD, operands
 * in registers), chip-wide TFLOP/s and the shader clock it settles at.  gfx950 clocks to its power budget: zero operands
 * reach the dense peak (~2.5 PFLOP/s at ~2.4 GHz), random fp16 operands -- what activations and weights are -- about two
 * thirds of it at ~1.6 GHz.  bench.py reports the conv roofline against the nominal peak AND against this measurement. */
int hp_probe_mfma_rate(int random_data, double* tflops, double* shader_mhz, void* stream);

/* ------------------------------------------------------------------------------------
 * Depth refinement (run_depth_refiner=True): point-to-plane ICP between the depth rendered at
 * the predicted pose and the measured depth.  Replaces icp_refinement / ICPRefiner.refine_poses
 * (MP/inference/icp_refiner.py:135-303, masks of MP/inference/refiner_utils.py:27-53); the
 * registration itself is OpenCV's ppf_match_3d_ICP there and a projective point-to-plane ICP here
 * (parity unpinned, see csrc/icp.hip).  d_depth_rendered [n][H][W] (hp_rasterize at d_TCO),
 * d_depth_measured [B][H][W] metres, d_masks [B][H][W] u8 or NULL (= the "threshold" mask with
 * depth_delta_thresh), im_ids on device and host, d_K [n][9].  Outputs: d_TCO_out [n][16]
 * (= input pose where the registration is rejected), d_retval [n] (0 / -1), d_residual [n]
 * (RMS point-to-plane distance of the inliers, metres, <= tolerance; -1 where rejected); the last
 * two may be NULL.
 * The two stages of an iteration on their own, through the launches hp_icp_refine makes:
 *  hp_icp_target_table: points and unit normals of d_depth_measured [B][H][W] with ONE row of
 *    d_K [B][9] per image -> d_tgt_out [B][H][W][6] (zeros where the depth is not > 0).
 *  hp_icp_accumulate: one pass over the pixels of n predictions with the caller's table d_tgt
 *    [B][H][W][6] and increments d_T [n][12] (rows of [R | t]; not read in mode 0) ->
 *    d_partial_out [n][64][32], the per-block sums whose fixed-order fp64 sum hp_icp_refine solves.
 *    mode 0: sums of the source points [0..2] and of the measured points at the same pixels
 *    [3..5], count [27].  mode 1: upper triangle of J^T J row by row [0..20], J^T r [21..26],
 *    count [27], sum r^2 [28].  Other entries are 0.  d_im_ids [n] must lie in 0 .. B-1 (on the
 *    device: not checked).
 * ---------------------------------------------------------------------------------- */
int hp_icp_refine(int n, int B, int H, int W, const float* d_depth_rendered, const float* d_depth_measured,
                  const uint8_t* d_masks, const int32_t* d_im_ids, const int32_t* h_im_ids, const float* d_K,
                  const float* d_TCO, int n_iterations, int n_min_points, float tolerance,
                  float depth_delta_thresh, float* d_TCO_out, int32_t* d_retval, float* d_residual,
                  void* stream);
int hp_icp_target_table(int B, int H, int W, const float* d_depth_measured, const float* d_K, float* d_tgt_out,
                        void* stream);
int hp_icp_accumulate(int n, int B, int H, int W, const float* d_depth_rendered, const float* d_depth_measured,
                      const uint8_t* d_masks, const int32_t* d_im_ids, const float* d_K, const float* d_tgt,
                      const float* d_T, int mode, float tolerance, float depth_delta_thresh, float* d_partial_out,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * Depth refinement, second kind (depth_refiner = "teaserpp"): robust registration between the depth rendered at the
 * predicted pose and the measured depth.  Replaces compute_teaserpp_refinement / TeaserppRefiner.refine_poses
 * (MP/inference/teaserpp_refiner.py:54-294); the solver is the teaserpp_python library there and a restatement of its
 * published definition here, with a deterministic GREEDY clique in place of the exact maximum clique (parity unpinned, see
 * csrc/teaser.hip for the definition).  Results are bit-identical from run to run.
 *  hp_teaser_fps: farthest-point sampling of n point sets, d_points [n][n_max][3], d_counts [n] points each: starts at
 *    index 0, takes the point farthest from the chosen set, ties to the lowest index.  d_indices [n][k]: min(k, count)
 *    indices in selection order, then -1.  d_scratch [n][n_max] floats.
 *  hp_teaser_register: b ~ R a + t for n sets of d_m[i] <= m_max <= 1024 correspondences, d_a / d_b [n][m_max][3].  d_T [n][16]
 *    (identity when rejected), d_status [n]: 0 accepted, -1 d_m[i] negative (the refinement's "too few masked pixels"),
 *    -2 clique smaller than 3, -3 fewer than min_num_inliers inliers (|R a + t - b| < noise_bound over the d_m[i]
 *    correspondences).  d_num_inliers [n], d_clique_size [n], d_clique_mask [n][32] (bit j of word w: correspondence
 *    32 w + j) may be NULL.
 *  hp_teaser_refine: the whole refinement, shaped like hp_icp_refine: mask (rendered > 0 & measured > 0, with
 *    use_threshold_mask also |measured - rendered| <= depth_delta_thresh), fewer than n_min_points pixels -> -1;
 *    back-projection x = (u - cx) d / fx, y = (v - cy) d / fy, z = d; min(n_points, N) correspondences by farthest-point
 *    sampling of the rendered points (use_farthest_point_sampling = 0: the evenly spaced indices floor(k N / M));
 *    registration; d_TCO_out = T d_TCO where accepted, d_TCO bit for bit otherwise.  d_num_inliers / d_clique_size may be
 *    NULL.  d_workspace: hp_teaser_workspace_bytes(n, H, W, n_points) bytes (-1 for sizes out of range: n_points 1 .. 1024).
 * ---------------------------------------------------------------------------------- */
int64_t hp_teaser_workspace_bytes(int n, int H, int W, int n_points);
int hp_teaser_fps(int n, int n_max, const float* d_points, const int32_t* d_counts, int k, float* d_scratch,
                  int32_t* d_indices, void* stream);
int hp_teaser_register(int n, int m_max, const float* d_a, const float* d_b, const int32_t* d_m, double noise_bound,
                       int min_num_inliers, float* d_T, int32_t* d_status, int32_t* d_num_inliers, int32_t* d_clique_size,
                       uint32_t* d_clique_mask, void* stream);
int hp_teaser_refine(int n, int B, int H, int W, const float* d_depth_rendered, const float* d_depth_measured,
                     const int32_t* d_im_ids, const int32_t* h_im_ids, const float* d_K, const float* d_TCO,
                     int use_threshold_mask, float depth_delta_thresh, int n_min_points, int n_points,
                     int use_farthest_point_sampling, double noise_bound, int min_num_inliers, float* d_TCO_out,
                     int32_t* d_retval, int32_t* d_num_inliers, int32_t* d_clique_size, void* d_workspace,
                     int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Detector stages that are not convolutions (the reference's Detector.get_detections, MP/inference/detector.py:34-156, runs
 * torchvision's MaskRCNN.forward; file references below are torchvision 0.14.1, pinned by the reference's pyproject.toml).
 * The dense networks are hp_net objects: HP_ARCH_RESNET50_FPN (backbone + FPN + RPN head) and two HP_ARCH_CUSTOM graphs
 * (box head, mask head).
 *  hp_rpn_decode: for the n anchors a pyramid level's top-k selected (d_anchor_idx = (y * map_w + x) * 3 + a, objectness
 *    logits gathered alongside): AnchorGenerator.grid_anchors (anchor_utils.py), BoxCoder.decode with weights (1,1,1,1) and
 *    the log(1000/16) clamp (_utils.py), clip_boxes_to_image, remove_small_boxes(min_size) as a validity flag, sigmoid
 *    (rpn.py: RegionProposalNetwork.filter_proposals).  d_deltas_map = that level's [h][map_w][12] map of ONE image.
 *  hp_nms: boxes sorted by decreasing score; h_keep[i] = 1 when box i survives greedy suppression (IoU > threshold) inside its
 *    group (ops/boxes.py: batched_nms).  Pairwise masks on the device, greedy pass on the host: SYNCHRONISES `stream`.
 *  hp_roi_align_levels: MultiScaleRoIAlign (ops/poolers.py): level k = floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to
 *    [k_min, k_min + n_levels), then roi_align(aligned=False) with spatial_scale h_scales[level] on that NHWC map
 *    [n_img][h][w][C]; d_rois [K][5] = image index, x1, y1, x2, y2 (image coordinates); d_out [K][out][out][C].
 *  hp_box_postprocess: softmax over n_classes + BoxCoder.decode with weights (10,10,5,5) per class + clip
 *    (roi_heads.py: postprocess_detections); d_scores [n][n_classes], d_boxes [n][n_classes][4].
 *  hp_paste_masks: maskrcnn_inference + paste_masks_in_image (roi_heads.py): sigmoid of channel d_labels[k] of the mask
 *    logits [n][14][14][2][2][ld] (the mask head's 2x2 deconvolution kept as four 1x1 convolutions), padding 1, box expanded
 *    and truncated to integers, bilinear resize (align_corners=False) to the box, pasted into d_out [n][H][W] (0 elsewhere).
 * ---------------------------------------------------------------------------------- */
int hp_rpn_decode(const float* d_objectness, const int32_t* d_anchor_idx, int n, const float* d_deltas_map, int map_w,
                  int n_anchors, const float* h_base_anchors /* [3][4] */, int stride_h, int stride_w, float im_h, float im_w,
                  float min_size, float* d_boxes, float* d_scores, uint8_t* d_valid, void* stream);
int hp_nms(const float* d_boxes, const int32_t* d_group, int n, float iou_threshold, uint8_t* h_keep, void* stream);
int hp_roi_align_levels(const float* const* h_feat_ptrs, const int* h_heights, const int* h_widths, const float* h_scales,
                        int n_levels, int k_min, int C, const float* d_rois, int K, int out_size, int sampling_ratio, float* d_out,
                        int32_t* d_levels /* [K] or NULL */, void* stream);
int hp_box_postprocess(const float* d_class_logits, int ld_logits, const float* d_box_regression, int ld_regression,
                       const float* d_proposals, int n, int n_classes, float im_h, float im_w, float* d_scores, float* d_boxes,
                       void* stream);
int hp_paste_masks(const float* d_mask_logits, int ld, const int32_t* d_labels, const float* d_boxes, int n, int H, int W,
                   float* d_out, void* stream);

/* Single layer entry (used by the parity tests of the conv kernels themselves):
 * y[n][ho][wo][cout] = act( conv(x_act, w) + bias + residual ),   act = relu: 0 none, 1 ReLU, 2 swish
 * x_act = x                                              (pre_scale == NULL)
 *       = relu(x * pre_scale[c] + pre_shift[c])           (both given: pre-activation BatchNorm, zero
 *                                                          padding AFTER it)
 *       = x * pre_scale[img][c]                           (pre_shift == NULL: squeeze-excitation gate
 *                                                          [n][cin] of an MBConv projection)
 * x NHWC [n][h][w][cin] (cin % 4 == 0), w packed [cout][kh][kw][cin] (cout % 4 == 0), stride 1|2,
 * symmetric padding.  The kernel family follows hp_conv_select_algo (Winograd / patch-staged direct
 * for 3x3 stride-1 layers with cin % 32 == 0 and cout % 64 == 0, the generic implicit GEMM else). */
int hp_conv2d_nhwc(const float* d_x, int n, int h, int w, int cin, const float* d_w, int cout,
                   int kh, int kw, int stride, int pad, const float* d_bias,
                   const float* d_residual, const float* d_pre_scale, const float* d_pre_shift,
                   int relu, float* d_y, void* stream);
/* the same for the fp16 kernel: x, w, residual, pre_scale / pre_shift and y are fp16 device
 * arrays (bias stays fp32); cin % 8 == 0, kh*kw*cin % 64 == 0, cout % 64 == 0 */
int hp_conv2d_nhwc_f16(const void* d_x, int n, int h, int w, int cin, const void* d_w, int cout, int kh,
                       int kw, int stride, int pad, const float* d_bias, const void* d_residual,
                       const void* d_pre_scale, const void* d_pre_shift, int relu, void* d_y,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-view scene reconstruction: the candidate matching of "consistent multi-view multi-object pose estimation"
 * (CP/multiview/ransac.py, CP/lib3d/symmetric_distances.py, CP/csrc/cosypose_cext.cpp).  csrc/multiview.hip.
 *
 * Mesh tables (MeshDataBase.batched(aabb=..., n_sym=...).to(device), CP/lib3d/rigid_mesh_database.py:27-78):
 * d_points [n_obj][n_pts][3] metres, d_symmetries [n_obj][s_max][16] (rows past an object's count are identity),
 * d_n_sym [n_obj] with 1 <= n_sym <= s_max.  Poses are [.][16].  Index columns are int32 on the device; an index
 * outside its table (or an n_sym outside 1..s_max) gives NaN in that row's output and reads nothing outside the tables.
 * One wavefront per row: results do not depend on launch geometry, no [rows][s_max] temporary exists.
 * ---------------------------------------------------------------------------------- */
#define HP_MV_DIST_3D 0
#define HP_MV_DIST_REPROJECTED 1
/* estimate_camera_poses (CP/multiview/ransac.py:23-50), one launch over all seeds.  For seed n with a = match1_cand1[n],
 * b = match1_cand2[n], g = match2_cand1[n], d = match2_cand2[n]: over the n_sym symmetries S of a's object, the distance of
 * symmetric_distance_batched_fast (below, itself minimised over the symmetries of g's object, on g's points) between
 * poses[g] and poses[a] S inv(poses[b]) poses[d]; the first strict minimum S* in symmetry order (scatter_argmin,
 * CP/csrc/cosypose_cext.cpp:220-247) gives d_TC1C2[n] = poses[a] S* inv(poses[b]). */
int hp_mv_estimate_camera_poses(int n_seeds, const int32_t* d_match1_cand1, const int32_t* d_match1_cand2,
                                const int32_t* d_match2_cand1, const int32_t* d_match2_cand2, const float* d_poses,
                                const int32_t* d_cand_obj, int n_cand, const float* d_points, const float* d_symmetries,
                                const int32_t* d_n_sym, int n_obj, int n_pts, int s_max, float* d_TC1C2, void* stream);
/* score_tmaches_batch / score_tmatches (CP/multiview/ransac.py:78-99), one launch over the tentative-match rows, gathered by
 * index on the device.  Row r: T1 = poses1[cand1[r]], T2 = TC1C2[hypothesis_id[r]] poses2[cand2[r]], object
 * obj1[cand1[r]].  (The matching passes the candidate table as poses1 and poses2.)
 *  HP_MV_DIST_3D: symmetric_distance_batched_fast (CP/lib3d/symmetric_distances.py:36-55): the symmetry S with the smallest
 *    MEAN OF SQUARED distances between (T1 S) p and T2 p over the object's points, lowest index on a tie; d_dists[r] is the
 *    MEAN OF THE ROOTS for that S.
 *  HP_MV_DIST_REPROJECTED: symmetric_distance_reprojected (:103-122) with d_K [n_hyp][9] indexed by hypothesis_id: the
 *    smallest mean L2 pixel distance of project_points (CP/lib3d/camera_geometry.py:4-18), first strict minimum.
 * d_sym_ids [n_rows] (may be NULL) receives the index of the chosen symmetry (-1 for a guarded row). */
int hp_mv_score_matches(int n_rows, const int32_t* d_hypothesis_id, const int32_t* d_cand1, const int32_t* d_cand2,
                        const float* d_TC1C2, int n_hyp, const float* d_poses1, const int32_t* d_obj1, int n_cand1,
                        const float* d_poses2, int n_cand2, const float* d_K, int mode, const float* d_points,
                        const float* d_symmetries, const int32_t* d_n_sym, int n_obj, int n_pts, int s_max, float* d_dists,
                        int32_t* d_sym_ids, void* stream);
/* The same 3D score for the rows of the candidate matching WITHOUT per-row index columns: every seed of a view pair lists all
 * tentative matches of that pair (make_ransac_infos), so the rows of seed n are d_row_offsets[n] .. d_row_offsets[n + 1]
 * ([n_seeds + 1], ascending from 0 to n_rows) and row r of them is match d_pair_offsets[n] + r - d_row_offsets[n] of the pair
 * tables d_pair_cand1 / d_pair_cand2 [n_pair_matches] (the tentative matches of each view pair once).  The only per-row device
 * memory is d_dists [n_rows].  A row outside the offsets or a match outside the pair tables gives NaN. */
int hp_mv_score_seed_matches(int n_rows, int n_seeds, const int32_t* d_row_offsets, const int32_t* d_pair_offsets,
                             const int32_t* d_pair_cand1, const int32_t* d_pair_cand2, int n_pair_matches, const float* d_TC1C2,
                             const float* d_poses, const int32_t* d_cand_obj, int n_cand, const float* d_points,
                             const float* d_symmetries, const int32_t* d_n_sym, int n_obj, int n_pts, int s_max, float* d_dists,
                             void* stream);
/* Body of MultiviewRefinement.forward_jacobian (CP/multiview/bundle_adjustment.py:223-270) without autograd, one wavefront per
 * candidate c with object o = cand_obj[c] and view v = cand_view[c]:  yhat = project(K[v], T(TCW_9d[v]) T(TWO_9d[o]) p),
 * y = project(K[v], TCO_cand[c] p) over the n_pts points of d_obj_points [n_obj][n_pts][3]; T(.) is
 * compute_transform_from_pose9d (CP/lib3d/transform_ops.py:57, Gram-Schmidt of TB/lib3d/rotations.py:22), differentiated
 * analytically (forward mode).  Outputs: d_errors [n_cand][n_pts][2] = y - yhat (UNCLIPPED: what the LM step uses),
 * d_clipped [n_cand][n_pts][2] = min(errors^2, residuals_threshold) (its mean is the loss), d_JtJ [n_cand][18][18] and
 * d_Jte [n_cand][18] = J^T J and J^T errors of the candidate, J = d yhat / d (9 object, 9 view parameters), summed over the points
 * in table order.  The caller adds the blocks into the full matrix in candidate order.  TCO_cand is the candidate's pose already
 * aligned by its symmetry (hp_mv_score_matches, HP_MV_DIST_REPROJECTED).  An o / v outside its table gives NaN outputs.
 * The parameters and the four outputs are DOUBLE (the host solves the normal equations in float64 and float32 blocks change the
 * LM run's accept / reject path on ill-conditioned scenes); candidate poses, K and points are the float32 tables. */
int hp_mv_ba_linearize(int n_cand, const double* d_TWO_9d, int n_obj, const double* d_TCW_9d, int n_views, const int32_t* d_cand_obj,
                       const int32_t* d_cand_view, const float* d_TCO_cand, const float* d_K, const float* d_obj_points, int n_pts,
                       double residuals_threshold, double* d_errors, double* d_clipped, double* d_JtJ, double* d_Jte, void* stream);
/* Host only (no device work).  make_ransac_infos (CP/csrc/cosypose_cext.cpp:38-107): tentative matches are the ordered pairs
 * (n, m) of candidates in different views with equal label ids; the view pairs are walked in ascending (view1, view2) order,
 * each with two permutations of its matches -- std::shuffle with std::default_random_engine(seed) and (seed + 1) -- and at
 * most n_ransac_iter seeds (pairs of distinct matches) per view pair; every seed lists all tentative matches of its view pair.
 * h_seeds [6][cap_seeds] = view1, view2, match1_cand1, match1_cand2, match2_cand1, match2_cand2; h_matches [3][cap_matches] =
 * hypothesis_id, cand1, cand2.  Call with both tables NULL to get the sizes, then with tables of at least those capacities. */
int hp_ransac_make_infos(int n_cand, const int32_t* h_view_ids, const int32_t* h_label_ids, int n_ransac_iter, int seed,
                         int64_t* n_seeds, int64_t* n_matches, int32_t* h_seeds, int64_t cap_seeds, int32_t* h_matches,
                         int64_t cap_matches);
/* find_ransac_inliers (CP/csrc/cosypose_cext.cpp:109-218).  Inliers of a hypothesis: matches with dist <= dist_threshold, made
 * one-to-one greedily by ascending distance (stable).  Per view pair (ascending order) the hypothesis with at least
 * n_min_inliers inliers wins that has more inliers, then the strictly smaller distance sum.  As in the reference a view pair is
 * kept only if the winning hypothesis id is > 0: hypothesis 0 -- the first seed of the first view pair -- can never be
 * selected.  That quirk is reproduced on purpose.  h_inlier_cand1 / h_inlier_cand2 hold up to n_matches entries,
 * h_best_hypotheses up to n_hyp. */
int hp_ransac_find_inliers(int64_t n_hyp, const int32_t* h_view1, const int32_t* h_view2, int64_t n_matches,
                           const int32_t* h_hypothesis_id, const int32_t* h_cand1, const int32_t* h_cand2, const float* h_dists,
                           float dist_threshold, int n_min_inliers, int32_t* h_inlier_cand1, int32_t* h_inlier_cand2,
                           int64_t* n_inliers, int32_t* h_best_hypotheses, int64_t* n_best);

/* ------------------------------------------------------------------------------------
 * Pose-error metrics of the evaluation: dists_add / dists_add_symmetric / dists_add_symmetries (TB/lib3d/distances.py),
 * chamfer_dist (CP/lib3d/symmetric_distances.py:58-78), the errors of PoseErrorMeter.compute_errors
 * (CP/evaluation/meters/pose_meters.py:60-116) and BOP's MSSD / MSPD.  csrc/pose_errors.hip.
 *
 * Row r is the triple (d_poses_pred[d_pred_id[r]], d_poses_gt[d_gt_id[r]], object d_obj_id[r]) with the mode d_mode[r]; the
 * four index columns are int32 [n_rows] on the device.  Mesh tables as in the multi-view section (d_points
 * [n_obj][max_pts][3], d_symmetries [n_obj][s_max][16], d_n_sym [n_obj]) plus d_n_pts [n_obj]: how many of the max_pts points of
 * an object count -- its own n_points for the reference's exact_meshes=True, max_pts for the padded table (padding repeats
 * vertices and the reference's non-exact mode counts them).  With p_j the object's points and d_j a per-point difference:
 *  HP_POSE_ERR_ADD      d_j = T_gt p_j - T_pred p_j
 *  HP_POSE_ERR_ADD_S    for every ground-truth point j the predicted point i with the smallest squared distance
 *                       dx^2 + dy^2 + dz^2 (computed from the differences, never from expanded norms), the lowest i on an exact
 *                       tie; d_j = T_gt p_j - T_pred p_i
 *  HP_POSE_ERR_ADD_SYM  over the object's n_sym symmetries S, T_gt S with the smallest mean |d_j| against T_pred (first strict
 *                       minimum); d_j for that S
 *  HP_POSE_ERR_MSSD     the S with the smallest max_j |T_pred p_j - T_gt S p_j| (first strict minimum); d_j for that S
 *  HP_POSE_ERR_MSPD     the same with both sides projected by d_K [n_rows][9] (project_points: K T p, divided by its third
 *                       component), d_j = (du, dv, 0) in pixels.  d_K may be NULL when no row asks for it.
 * ADD(-S) is not a mode: the caller sets ADD or ADD-S per row from the object's is_symmetric.
 * n_add_s: how many rows are ADD-S if the caller knows it, negative if it does not.  0 skips the ADD-S launches (blocks x n_rows
 * workgroups that would only read the index columns) and needs no workspace; an ADD-S row in such a call is answered like a
 * guarded row.
 * Outputs per row: d_norm_avg = mean |d_j|, d_xyz_avg [.][3] = mean of the absolute components, d_norm_max = max |d_j| (for MSSD
 * and MSPD this IS the metric), d_sym_id = the chosen symmetry (-1 in ADD and ADD-S), d_TCO_xyz [.][3] = |t_pred - t_gt| and
 * d_TCO_norm its length.  d_assign [n_rows][max_pts] (may be NULL): in ADD-S the chosen i of every j, in every other mode j; -1
 * past the object's n_pts.
 * An index outside its table, an n_sym outside 1..s_max, an n_pts outside 1..max_pts, an unknown mode or MSPD without d_K
 * give NaN in every float output of that row (sym_id and assign -1); such a row reads nothing outside the tables.
 * n_rows == 0 returns HP_OK before anything else is looked at and launches nothing; at most 65535 rows per call.
 * ADD-S: a workgroup is one (row, block of HP_POSE_ERR_GT_BLOCK ground-truth points), the predicted points pass through LDS in
 * tiles of HP_POSE_ERR_PRED_TILE; per-block partial sums go to d_workspace (hp_pose_errors_workspace_bytes(n_rows, max_pts)
 * bytes: n_rows x blocks x 32, nothing of size max_pts^2) and are added in block order.  No atomics: a row's outputs do not depend
 * on the other rows of the call and are bit-identical from run to run.
 * ---------------------------------------------------------------------------------- */
#define HP_POSE_ERR_ADD 0
#define HP_POSE_ERR_ADD_S 1
#define HP_POSE_ERR_ADD_SYM 2
#define HP_POSE_ERR_MSSD 3
#define HP_POSE_ERR_MSPD 4
#define HP_POSE_ERR_PRED_TILE 512
#define HP_POSE_ERR_GT_BLOCK 1024
int64_t hp_pose_errors_workspace_bytes(int n_rows, int max_pts);
int hp_pose_errors(int n_rows, const int32_t* d_pred_id, const int32_t* d_gt_id, const int32_t* d_obj_id, const int32_t* d_mode,
                   int n_add_s, const float* d_poses_pred, int n_pred, const float* d_poses_gt, int n_gt, const float* d_K,
                   const float* d_points, const float* d_symmetries, const int32_t* d_n_sym, const int32_t* d_n_pts, int n_obj,
                   int max_pts, int s_max, float* d_norm_avg, float* d_xyz_avg, float* d_norm_max, int32_t* d_sym_id,
                   float* d_TCO_xyz, float* d_TCO_norm, int32_t* d_assign, void* d_workspace, int64_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------
 * The losses the pose networks are trained and validated on, value and gradient: loss_CO_symmetric
 * (TB/lib3d/cosypose_ops.py:65-79 = CP/lib3d/cosypose_ops.py:45-59), compute_ADD_L1_loss (TB/lib3d/mesh_losses.py:39-48),
 * loss_refiner_CO_disentangled (CP/lib3d/cosypose_ops.py:62-101) and loss_refiner_CO_disentangled_reference_point
 * (TB/lib3d/cosypose_ops.py:82-156), the validation figure loss_TCO-iter=k of the reference's trainers.  csrc/pose_losses.hip.
 * There is no trainer here: this is the loss layer.
 *
 * Row b of B holds d_TCO_possible_gt [b][n_sym][16] (entry 0 is the ground truth) and d_points [b][n_pts][3].
 * The symmetric loss of a pose T_pred: for every symmetry s, l_s = mean over the points j and the three components of
 * |T_pred p_j - T_gt,s p_j|; the loss is min_s l_s and the chosen s the lowest index on an exact tie.  compute_ADD_L1_loss is the
 * same with n_sym = 1.  hp_loss_co_symmetric writes d_loss [b], d_sym_id [b] and, unless NULL, d_TCO_assign [b][16] = the chosen
 * T_gt,s.
 * The disentangled refiner loss of the network's 9-D update o (d_refiner_outputs [b][9]: 6-D rotation, vx vy, vz) at the input
 * pose d_TCO_input [b][16] with the crop's intrinsics d_K_crop [b][9] (fx = K[0], fy = K[4]) is the sum of three symmetric losses,
 * each with its own minimum over s, of three poses that are the ground truth T_gt = T_gt,0 except for
 *   orientation  the rotation dR R_in, dR = compute_rotation_matrix_from_ortho6d(o[0:6]) (Gram-Schmidt, no epsilon)
 *   xy           t_x, t_y of the update applied with the ground truth's rotation update and depth ratio
 *   z            t_z of the update applied with the ground truth's rotation update.
 * d_tCR == NULL, CosyPose's image-space update: t_xy = (o[6:8] / fxfy + t_in,xy / t_in,z) t_gt,z and t_z = o[8] t_in,z.
 * d_tCR [b][3], MegaPose's update about the reference point: with dR_gt = R_gt R_in^T, q = dR_gt (t_in - tCR) and
 * vz_gt = (t_gt,z - q_z) / tCR_z: t_xy = q_xy + (o[6:8] / fxfy + tCR_xy / tCR_z) vz_gt tCR_z and t_z = q_z + o[8] tCR_z (the
 * reference's vxvy_gt reaches none of the three poses).
 * hp_loss_refiner_disentangled writes d_loss [b] = orn + xy + z, d_loss_parts [b][3] = (loss_orn, loss_xy, loss_z) and
 * d_sym_ids [b][3], the symmetry each term chose.
 *
 * Gradients: of the symmetric loss with respect to the upper 3 x 4 of T_pred (d_grad_TCO_pred [b][16], last row zero), of the
 * refiner loss with respect to o only (d_grad_outputs [b][9]; the reference detaches TCO_input between iterations, the rest is
 * data), both multiplied by the row's upstream gradient d_grad_loss [b].  The gradient flows through the chosen symmetry only
 * (d_sym_id / d_sym_ids as the forward call wrote them), d|x|/dx = sign(x) with sign(0) = 0, the orientation term chains
 * through the Gram-Schmidt, the xy term reaches o[6], o[7] only and the z term o[8] only.  d_grad_parts [b][3][9] (may be NULL)
 * receives the same gradient split by term.
 *
 * The points are transformed in float32; the predicted poses and every sum are formed in double and rounded once.  A term loss
 * that is not finite -- a non-finite point, pose, intrinsic or update, a degenerate 6-D part -- makes every float output of the row
 * NaN and its ids -1, and the backward call answers ids outside 0..n_sym-1 with a NaN gradient row; other rows are untouched.
 * b == 0 returns HP_OK and launches nothing; n_sym < 1 or n_pts < 1 is HP_ERR_ARG.  A workgroup is one (row, chunk of
 * HP_POSE_LOSS_SYM_CHUNK symmetries); the per-(row, symmetry, term) means go to d_workspace (hp_pose_loss_workspace_bytes(b,
 * n_sym) bytes = b x n_sym x 12, nothing of size b x n_sym x n_pts) and a second launch takes the minima.  The backward calls
 * need no workspace.  No atomics: a row's outputs do not depend on the other rows of the call and are bit-identical from run to run.
 * ---------------------------------------------------------------------------------- */
#define HP_POSE_LOSS_SYM_CHUNK 8
int64_t hp_pose_loss_workspace_bytes(int b, int n_sym);
int hp_loss_co_symmetric(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_pred, const float* d_points,
                         float* d_loss, int32_t* d_sym_id, float* d_TCO_assign, void* d_workspace, int64_t workspace_bytes,
                         void* stream);
int hp_loss_co_symmetric_backward(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_pred,
                                  const float* d_points, const int32_t* d_sym_id, const float* d_grad_loss, float* d_grad_TCO_pred,
                                  void* stream);
int hp_loss_refiner_disentangled(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_input,
                                 const float* d_refiner_outputs, const float* d_K_crop, const float* d_points,
                                 const float* d_tCR /* [b][3] or NULL */, float* d_loss, float* d_loss_parts, int32_t* d_sym_ids,
                                 void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_loss_refiner_disentangled_backward(int b, int n_sym, int n_pts, const float* d_TCO_possible_gt, const float* d_TCO_input,
                                          const float* d_refiner_outputs, const float* d_K_crop, const float* d_points,
                                          const float* d_tCR /* [b][3] or NULL */, const int32_t* d_sym_ids,
                                          const float* d_grad_loss, float* d_grad_outputs, float* d_grad_parts, void* stream);
/* The rendered-views-logits loss of the coarse classifier (MP/training/megapose_forward_loss.py:224-239):
 * nn.BCEWithLogitsLoss(reduction="none") of x = logit / temperature against the target y (0 / 1; any value in [0, 1] is accepted),
 * per element:  loss = max(x, 0) - x y + log1p(exp(-|x|)),  d loss / d logit = (sigmoid(x) - y) / temperature, the backward call
 * multiplies it by the element's upstream gradient d_grad_loss.  Evaluated in double from the float32 inputs and rounded once; no
 * overflow for any finite logit.  n elements, n == 0 launches nothing; temperature <= 0 or not finite is HP_ERR_ARG. */
int hp_loss_bce_logits(int64_t n, const float* d_logits, const float* d_targets, float temperature, float* d_loss, void* stream);
int hp_loss_bce_logits_backward(int64_t n, const float* d_logits, const float* d_targets, float temperature, const float* d_grad_loss,
                                float* d_grad_logits, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-object scenes:Panda3dSceneRenderer.render_scene(object_datas, camera_datas, light_datas, ...)
 * (TB/renderer/panda3d_scene_renderer.py:320-390), the gt-info quantities of MP/scripts/bop_calc_gt_info.py (px_count_all,
 * px_count_visib, bbox_obj, bbox_visib), make_contour_overlay (TB/visualization/utils.py:54-82) and BokehPlotter.plot_overlay
 * (TB/visualization/bokeh_plotter.py:116-141).  csrc/scene.hip.
 *
 * hp_rasterize draws one object per view, so a scene is rendered as LAYERS: one view per (camera, object) pair, sorted by
 * camera.  d_layer_off [n_cam + 1] (device, int32) holds every camera's range into the layer buffers; all cameras of a call share
 * h x w.  The layer buffers are NCHW as hp_rasterize writes them: d_layer_rgb [n_layers][3][h][w], d_layer_nrm the same or NULL,
 * d_layer_depth [n_layers][1][h][w] in metres with 0 = background.  A camera may own no layer.  Offsets are clamped into
 * [0, n_layers] on the device: a corrupt table reads nothing outside the buffers.
 *
 * hp_scene_compose: at every pixel the winner is the layer of that camera with the smallest depth > 0, the LOWEST layer on a tie
 * (NaN and +inf never win).  d_rgb [n_cam][3][h][w], d_nrm the same (NULL: not wanted; needs d_layer_nrm), d_depth
 * [n_cam][1][h][w], d_ids [n_cam][h][w] int32 = the winner's index WITHIN its camera, d_mask [n_cam][1][h][w] u8.  Without a
 * winner: colour, normals and depth 0, id -1, mask 0.  Values are copies of the winner's -- no arithmetic -- so the outputs are a
 * bit-exact function of the layers.
 * LIMITATION: every layer was resolved on its own, 4x multisampled against black (HP_RASTER_MSAA4): where the silhouette of a
 * nearer object crosses a farther one, the nearer layer's edge pixels blend with black instead of with the object behind, in a
 * band at most one pixel wide.  Depth, ids, mask and visibility are exact; single-sampled layers compose to exactly the colours
 * of one shared z-buffer.
 *
 * hp_scene_visibility: d_table [n_layers][HP_SCENE_VIS_FIELDS] int32 = px_count_all (layer depth > 0), px_count_visib (d_ids of
 * the layer's camera equals the layer's index within it), bbox_all (x_min, y_min, x_max, y_max inclusive), bbox_visib (the same of
 * the visible pixels); every field of a box whose count is 0 is -1.  The call initialises the table, then counts with integer
 * atomics: the result does not depend on the launch order.  visib_fract = px_count_visib / px_count_all is the host's division.
 *
 * hp_scene_contour: d_out [n_cam][h][w][3] u8 = d_frame with the outline painted in (color_r, color_g, color_b), d_edge
 * [n_cam][h][w] u8 (may be NULL) = 255 on the outline, else 0.  The region is given by exactly one of d_mask [n_cam][h][w] u8
 * (non-zero = inside) and d_ids [n_cam][h][w] int32 (>= 0 = inside).  Definition (this library's own: the reference runs
 * cv2.Canny on the binary mask and dilates with a 3 x 3 kernel, which cannot be pinned without OpenCV):
 *   edge0[p]  p is inside and at least one of its 4-neighbours INSIDE THE IMAGE is outside the region -- with per_object != 0
 *             (d_ids only): has a different id;
 *   edge[p]   some q with Chebyshev distance <= dilate_iterations from p has edge0[q].
 * dilate_iterations in 0..HP_SCENE_MAX_DILATE, anything else is HP_ERR_ARG.  One launch; d_out must not alias d_frame.
 *
 * hp_scene_overlay: d_out = where the render is set: d_lut_render[render], elsewhere d_lut_input[input], per byte of the
 * [n_cam][h][w][3] u8 frames.  "Set" = d_mask [n_cam][h][w] != 0 when given, else any channel of the render pixel > 0 (the
 * reference's get_mask_from_rgb).  The two 256-entry u8 tables (device) hold render * 0.8 + 255 * 0.2 and input * 0.6 + 255 * 0.4
 * as numpy evaluates and truncates them (happypose_amd.scene.overlay_tables).
 * n_cam == 0 launches nothing.
 * ---------------------------------------------------------------------------------- */
#define HP_SCENE_VIS_FIELDS 10
#define HP_SCENE_MAX_DILATE 3
int hp_scene_compose(int n_cam, const int32_t* d_layer_off, int n_layers, int h, int w, const float* d_layer_rgb,
                     const float* d_layer_nrm, const float* d_layer_depth, float* d_rgb, float* d_nrm, float* d_depth, int32_t* d_ids,
                     uint8_t* d_mask, void* stream);
int hp_scene_visibility(int n_cam, const int32_t* d_layer_off, int n_layers, int h, int w, const float* d_layer_depth,
                        const int32_t* d_ids, int32_t* d_table, void* stream);
int hp_scene_contour(int n_cam, int h, int w, const uint8_t* d_frame, const uint8_t* d_mask, const int32_t* d_ids, int per_object,
                     int color_r, int color_g, int color_b, int dilate_iterations, uint8_t* d_out, uint8_t* d_edge, void* stream);
int hp_scene_overlay(int n_cam, int h, int w, const uint8_t* d_input, const uint8_t* d_render, const uint8_t* d_mask,
                     const uint8_t* d_lut_render, const uint8_t* d_lut_input, uint8_t* d_out, void* stream);

/* ------------------------------------------------------------------------------------
 * BOP's visible-surface discrepancy (VSD) in its BOP19 form: visibility mode "bop19", cost "step".  The reference leaves it to
 * bop_toolkit (pose_error.vsd with misc.depth_im_to_dist_im_fast and visibility.estimate_visib_mask_gt / _est); the definition
 * is restated here in full.  csrc/vsd.hip.
 *
 * Row r compares the depth render d_depth_layers[d_est_layer[r]] (the object at the estimated pose) and
 * d_depth_layers[d_gt_layer[r]] (at the ground-truth pose) with the measured depth image d_depth_test[d_frame[r]] under the
 * intrinsics d_K[d_frame[r]]; d_diameter[r] is the object's diameter.  All images are [.][h][w] float32 in metres, 0 = no
 * measurement / background (hp_rasterize's depth output: a pixel is covered iff its centre is); d_K is [n_frames][9]; the three
 * index columns are int32 [n_rows] and d_diameter float32 [n_rows], on the device.  Many rows may name one layer: a ground-truth
 * render serves every estimate matched against it.  With D_t, D_e, D_g the three depths of pixel (u, v) (column, row; integer
 * indices, no half-pixel offset):
 *   f(u, v) = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1),   S_x = D_x f   (the distance images)
 *   V_g = S_g > 0 and (S_g - S_t <= delta or S_t == 0)
 *   V_e = (S_e > 0 and (S_e - S_t <= delta or S_t == 0)) or (V_g and S_e > 0)
 *   I = V_g and V_e,  U = V_g or V_e,  n_I = |I|,  n_U = |U|
 *   c_tau = the number of pixels of I with |S_g - S_e| / d >= tau, d = d_diameter[r] if normalized_by_diameter else 1
 *   e_tau = (c_tau + n_U - n_I) / n_U, and 1 when n_U == 0.
 * f and the S_x are float32 (one f per pixel, applied to the three depths); a pixel within a few float32 roundings of a threshold
 * may fall on either side of it.  Everything accumulated is an integer.
 * Outputs: d_counts [n_rows][HP_VSD_COUNT_FIELDS] int32 = n_U, n_I, |V_e|, |V_g|; d_cost [n_rows][n_tau] int32 = c_tau; d_errors
 * [n_rows][n_tau] float32 = e_tau, the integer quotient rounded once.  taus is a HOST array of n_tau values,
 * 1 <= n_tau <= HP_VSD_MAX_TAUS; d_diameter may be NULL without normalized_by_diameter and must be positive with it.
 * The ids in the three index columns MUST be in range (0 <= layer < n_layers, 0 <= frame < n_frames): the caller checks them
 * where they still live on the host.  The kernels do compare them with the table sizes: a row with an id outside reads no image
 * and is answered with -1 in its counts and cost and NaN in its errors.
 * One pass over the pixels, a workgroup per (row, block of 4096 pixels), 16-byte loads when h * w is a multiple of 4 and the
 * image buffers are 16-byte aligned; every workgroup leaves one record of integers in d_workspace
 * (hp_vsd_workspace_bytes(n_rows, h, w) bytes: n_rows x ceil(h w / 4096) x 80), added per row in block order by a second launch.
 * No atomics: a row's outputs do not depend on the other rows of the call, on their order or on the run.
 * n_rows == 0 returns HP_OK after the scalar checks and launches nothing; h * w < 2^31 and at most 65535 pixel blocks per
 * frame.  hp_vsd_workspace_bytes returns -1 for a negative n_rows or a frame outside those limits.
 * ---------------------------------------------------------------------------------- */
#define HP_VSD_MAX_TAUS 16
#define HP_VSD_COUNT_FIELDS 4
int64_t hp_vsd_workspace_bytes(int n_rows, int h, int w);
int hp_vsd(int n_rows, const int32_t* d_est_layer, const int32_t* d_gt_layer, const int32_t* d_frame, const float* d_diameter,
           const float* d_depth_test, int n_frames, const float* d_depth_layers, int n_layers, const float* d_K, int h, int w,
           float delta, int n_tau, const float* taus, int normalized_by_diameter, int32_t* d_counts, int32_t* d_cost,
           float* d_errors, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Scoring 2D detections and instance masks: box IoU, mask IoU and COCO's greedy matching.  The reference has DetectionMeter
 * (CP/evaluation/meters/detection_meters.py: torchvision's box_iou at one threshold); BOP scores its 2D detection and 2D
 * segmentation tasks with COCO average precision, which the reference leaves to pycocotools.  The definitions below are the
 * PUBLISHED ones (torchvision 0.14.1 ops.box_iou; COCOeval.evaluateImg of pycocotools 2.0) restated here in full: neither package
 * is a dependency, so nothing here could be pinned against them.  csrc/det_eval.hip.
 *
 * hp_mask_pack: d_masks [n][h w] uint8 (non-zero = set; the storage of a bool tensor qualifies) -> d_words [n][W64] uint64 and
 * d_area [n] int32.  W64 = hp_mask_pack_words(h, w) = ceil(h w / 64); bit i of word k is pixel 64 k + i of the flattened plane; the
 * unused high bits of the last word are 0; d_area[m] is the number of set pixels of mask m.  h w <= 2^24, so that every count is
 * exact in float32 (hp_mask_pack_words returns -1 outside).  8-byte loads when h w is a multiple of 8 and d_masks is 8-byte aligned
 * (8 lanes fold their bytes into one word), else byte loads and one wavefront ballot per word.  d_area is zeroed on the stream and
 * receives one integer atomic per workgroup.
 *
 * hp_det_iou: row r compares prediction d_pred_idx[r] with ground truth d_gt_idx[r] (int32 [n_rows], device; 0 <= id < n_pred /
 * n_gt -- the caller checks them where they still live on the host; a row with an id outside reads nothing and is answered with
 * NaN IoUs and -1 counts).  Either input family may be NULL, which skips that part and its outputs.
 *   boxes  d_boxes_pred [n_pred][4], d_boxes_gt [n_gt][4] float32 (x1, y1, x2, y2):
 *            area = (x2 - x1) (y2 - y1),  wh = max(min(rb) - max(lt), 0),  inter = w h,  iou = inter / (a1 + a2 - inter)
 *          in float32; 0 / 0 stays NaN.  d_box_iou [n_rows] float32.
 *   masks  d_words_* / d_area_* as hp_mask_pack writes them, w64 words per mask:
 *            inter = sum_k popcount(words_pred[k] & words_gt[k]),  union = area_pred + area_gt - inter  (int32: d_inter, d_union)
 *            d_mask_iou = (float)inter / (float)union, the correctly rounded float32 quotient; 0 where union == 0.
 * One workgroup per row, integers only: a row's outputs depend on its two masks alone, not on the other rows, their order or the
 * run.  Rows are in grid x: any n_rows >= 0 works, n_rows == 0 launches nothing.
 *
 * hp_det_match: COCO's greedy matching.  Group g (one image and label) owns the dense IoU matrix d_iou[d_row_off[g] + d n_gt[g] + j]
 * of its n_det[g] detections x n_gt[g] ground truths, detection-major; its outputs start at d_det_off[g] / d_gt_off[g].  All group
 * tables are int32 [n_groups] on the device, d_gt_ignore is uint8 [total_gts], d_thr float32 [n_thr] (device).  The HOST has ordered
 * each group: detections by descending score (stable, capped at max_dets), ground truths with the non-ignored ones first (stable).
 * Rule per threshold, for the detections in order:
 *   - Among ground truths not yet matched at this threshold, consider the non-ignored ones with iou >= thr and take the largest IoU.
 *   - Only if there is none, do the same among the ignored ones.
 *   - An exact tie goes to the ground truth with the higher position.  This is pycocotools' loop with its `<` comparison.
 *   - The comparison is `>=` in float32 against thr as passed.  The host passes float32(min(t, 1 - 1e-10)).
 *   - A detection matched to an ignored ground truth is itself ignored.  NaN IoUs never match.
 * Outputs: d_det_match [n_thr][total_dets] int32 = the ground truth's position in its group or -1; d_det_ignore [n_thr][total_dets]
 * uint8; d_gt_match [n_thr][total_gts] int32 = the detection's position in its group or -1.  One wavefront per (group, threshold),
 * lanes strided over the ground truths (any n_gt), detections sequential.  Groups with n_det == 0 or n_gt == 0 are legal.  A group
 * whose ranges leave the tables (total_rows, total_dets, total_gts) touches nothing.
 * ---------------------------------------------------------------------------------- */
int64_t hp_mask_pack_words(int h, int w);
int hp_mask_pack(int n, int h, int w, const uint8_t* d_masks, uint64_t* d_words, int32_t* d_area, void* stream);
int hp_det_iou(int n_rows, const int32_t* d_pred_idx, const int32_t* d_gt_idx, int n_pred, int n_gt, const float* d_boxes_pred,
               const float* d_boxes_gt, const uint64_t* d_words_pred, const int32_t* d_area_pred, const uint64_t* d_words_gt,
               const int32_t* d_area_gt, int w64, float* d_box_iou, int32_t* d_inter, int32_t* d_union, float* d_mask_iou,
               void* stream);
int hp_det_match(int n_groups, const int32_t* d_n_det, const int32_t* d_n_gt, const int32_t* d_row_off, const int32_t* d_det_off,
                 const int32_t* d_gt_off, const float* d_iou, int64_t total_rows, int64_t total_dets, int64_t total_gts,
                 const uint8_t* d_gt_ignore, const float* d_thr, int n_thr, int32_t* d_det_match, uint8_t* d_det_ignore,
                 int32_t* d_gt_match, void* stream);

/* ------------------------------------------------------------------------------------
 * Mesh surface resampling: the point table of MeshDataBase.batched(resample_n_points=N) (TB/lib3d/rigid_mesh_database.py:96-99,
 * CP/lib3d/rigid_mesh_database.py:38-40) and of ModelNetErrorMeter.  The reference calls trimesh.sample.sample_surface; trimesh
 * is not a dependency, so parity with it is UNPINNED and the definition below is the whole contract.  It is trimesh's documented
 * algorithm (a face is picked with probability proportional to its area, the point is uniform in that face by the
 * reflected-parallelogram rule) with two deliberate differences, marked (*).  csrc/mesh_sample.hip.
 *
 * Tables: the vertices (d_vertices [total_verts][3] float32) and faces (d_faces [total_faces][3] int32, indices LOCAL to their
 * object) of all objects packed back to back; d_vert_offset / d_face_offset [n_obj + 1] int32 on the device give object o the rows
 * offset[o] .. offset[o + 1].  With V and F the object's counts:
 *  Areas and CDF   area_f = 0.5 |(v1 - v0) x (v2 - v0)| in fp64 from the fp32 vertices: e = v - v0 per component, the cross product
 *                  as (ay bz - az by, az bx - ax bz, ax by - ay bx), the norm as sqrt((cx cx + cy cy) + cz cz), every operation
 *                  rounded once (no fused multiply-add).  cum[f] = the inclusive prefix sum in fp64, in a FIXED order: one
 *                  workgroup per object, chunks of 1024 faces in sequence with a carried prefix (wavefront scan, wave totals added
 *                  in wave order).  No atomics, bit-identical from run to run; it differs from the sequential sum by rounding
 *                  only (about F 2^-53 relative).  total = cum[F - 1] goes to d_area [n_obj] (may be NULL).
 *  Random numbers  sample i of object o draws Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key
 *                  increments 0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and counter (i, o, 0, 0), giving
 *                  r0..r3.  Stateless: a sample does not depend on n_samples, on n_obj or on the other objects of the call.
 *  Face pick       u = ((uint64)r0 << 21 | r1 >> 11) 2^-53,  pick = u total  in fp64; the face is the first f with cum[f] > pick
 *                  (STRICT), by binary search, clamped to F - 1.
 *                  (*) trimesh uses searchsorted(side="left") (cum[f] >= pick): the strict rule never picks a zero-area face,
 *                  except through the clamp.
 *  Point           ia = r2 >> 8, ib = r3 >> 8 (24-bit integers); if ia + ib > 2^24 both become 2^24 - i -- (*) compared on the
 *                  integers: trimesh's float a + b > 1 may round; a = ia 2^-24, b = ib 2^-24 (exact in fp32);
 *                  p = (v0 + a (v1 - v0)) + b (v2 - v0)  per component in fp32, every operation rounded once.
 *                  d_points [n_obj][n_samples][3], d_face_id [n_obj][n_samples] (object-local, may be NULL).
 *  Guards          an object with no faces, total == 0, a non-finite total, a face index outside 0 .. V - 1, or offsets that are
 *                  negative, descend or pass the table the workspace was sized for gives NaN points and face_id -1 for all its
 *                  samples (d_area: the total, NaN for bad indices or offsets).  Such an object reads nothing outside the tables:
 *                  a face with a bad index reads no vertex.  Its neighbours in the call are unaffected.
 * n_obj == 0 or n_samples == 0 returns HP_OK and launches nothing.  At most 65535 objects per call, total_faces < 2^31.
 * d_workspace: hp_mesh_sample_workspace_bytes(n_obj, total_faces) = 8 (n_obj + total_faces) bytes, 8-byte aligned (-1 for sizes
 * out of range): the totals and the CDF.  Two kernels (areas + scan, then one thread per (object, sample)), wave64, no
 * floating-point atomics; not used on the render-and-compare path.
 * ---------------------------------------------------------------------------------- */
int64_t hp_mesh_sample_workspace_bytes(int n_obj, int64_t total_faces);
int hp_mesh_sample_surface(int n_obj, const float* d_vertices, const int32_t* d_faces, const int32_t* d_vert_offset,
                           const int32_t* d_face_offset, int n_samples, uint64_t seed, float* d_points, int32_t* d_face_id,
                           double* d_area, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Training-image augmentations: the transforms of the reference's toolbox/datasets/augmentations.py on a whole batch of frames
 * that already lives on the device.  csrc/augment.hip; the user-facing layer is happypose_amd/augmentations.py.
 *
 * Tensors are dense: d_rgb / d_background / d_out [B][h][w][3] uint8; d_depth [B][h][w] float32 in metres, 0 = invalid;
 * d_segmentation [B][h][w] int32, 0 = background.  Every per-image parameter is a DEVICE array of length B; d_apply [B] uint8:
 * an image with d_apply[b] == 0 comes back bit for bit.  The result for image b does not depend on the other images or on B.
 * There are no floating-point atomics: results are bit-identical from run to run.  B == 0 returns HP_OK and launches nothing;
 * a null pointer, h <= 0, w <= 0, B > 65535 or h w > 2^28 is HP_ERR_ARG before the GPU is touched.
 * IN PLACE (d_out == d_rgb / d_depth) is allowed for hp_aug_replace_background, hp_aug_depth_noise, hp_aug_depth_missing,
 * hp_aug_depth_ellipses and hp_aug_depth_mask; hp_aug_rgb_enhance, hp_aug_rgb_blur and hp_aug_depth_blur read a neighbourhood and
 * answer HP_ERR_ARG when d_out aliases the input.
 * d_workspace: hp_aug_workspace_bytes(B, h, w, max_ellipses) = 8 B + roundup8(4 B h w) + 32 B max_ellipses bytes, 8-byte aligned
 * (-1 for sizes out of range); max_ellipses is 0 for every call but hp_aug_depth_ellipses.  hp_aug_replace_background,
 * hp_aug_depth_blur, hp_aug_depth_mask and uncorrelated hp_aug_depth_noise use none.
 *
 * RGB: Pillow's arithmetic, matched byte for byte (pinned against Pillow 12.2 by tests/golden/g14_augmentations.npz).
 *   blend(a, x, f)   per byte in float32, every operation rounded once (no fused multiply-add): t = a + f (x - a).  For
 *                    0 <= f <= 1 the result is (uint8) t, truncated; otherwise t <= 0 gives 0, t >= 255 gives 255, else truncated.
 *   gray             (R 19595 + G 38470 + B 7471 + 0x8000) >> 16.
 *   hp_aug_rgb_enhance, d_op[b] one of HP_AUG_OP_* (any other value leaves the image unchanged), d_factor[b] = f:
 *     BRIGHTNESS     blend(0, x, f)
 *     COLOR          blend(gray, x, f), the pixel's gray in all three channels
 *     CONTRAST       blend(m, x, f), m = (int)(sum(gray) / (double)(h w) + 0.5): one scalar per image; the sum is an exact 64-bit
 *                    integer (integer atomics, one per workgroup), the division is done in double
 *     SHARPNESS      blend(smooth(x), x, f); smooth is Pillow's SMOOTH: the 3 x 3 kernel (1,1,1,1,5,1,1,1,1), each tap the float32
 *                    of k / 13, accumulated in float32 onto an initial 0.5 -- row y + 1 first, then y, then y - 1, each from left to
 *                    right, every product and sum rounded once -- then floor and clip to 0..255.  The one-pixel border is copied
 *                    unchanged; an image with h < 3 or w < 3 is all border.
 *   hp_aug_rgb_blur  Pillow's GaussianBlur of integer radius k as three box passes along the rows, then three along the columns,
 *                    EVERY pass rounded to uint8.  The HOST computes per image, in float32: sigma2 = k k / 3,
 *                    L = sqrt(12 sigma2 + 1), l = floor((L - 1) / 2), a = (2 l + 1)(l (l + 1) - 3 sigma2) / (6 (sigma2 - (l + 1)^2)),
 *                    r_f = l + a (0.25000003, 1.375, 2.4166667 for k = 1, 2, 3); d_radius = r = (int) r_f,
 *                    d_ww = (uint32)(2^24 / (2 r_f + 1)) in float32, d_fw = (2^24 - (2 r + 1) ww) / 2.  One pass along a line is
 *                      out[x] = (ww sum_{i = -r..r} in[clamp(x + i)] + fw (in[clamp(x - r - 1)] + in[clamp(x + r + 1)]) + 2^23) >> 24
 *                    in 32-bit unsigned integers, indices clamped to the line.  A line of at most 1024 pixels runs its three
 *                    passes in the LDS (rows: one workgroup per line; columns: one per 8 columns); a longer one, or every one
 *                    with force_general != 0, takes one launch per pass through the workspace.  Both paths give the same bytes.
 *   hp_aug_replace_background   out = background where segmentation == 0, else rgb.  d_background is already at frame size.
 *
 * Depth: the reference's definitions restated; it calls OpenCV (resize, ellipse, blur), which is not a dependency, so parity with
 * OpenCV is UNPINNED and what follows is the whole contract.  The reference's random streams (the global `random` / `np.random`
 * state) are not reproduced either.
 *   Random numbers   Philox4x32-10 as for hp_mesh_sample_surface, key (seed & 0xffffffff, seed >> 32), counter
 *                    (index, b, stream, 0): index = the pixel's row-major index in its image, or the cell's in its grid; b = the
 *                    image's index in the call; stream = HP_AUG_STREAM_NOISE (1), _GRID (2) or _MISSING (3).  A normal deviate is
 *                    Box-Muller in float32 on words r0, r1: u1 = ((r0 >> 8) + 1) 2^-24 in (0, 1], u2 = (r1 >> 8) 2^-24,
 *                    n = sqrt(-2 ln u1) cos(6.2831855f u2).
 *   hp_aug_depth_noise, correlated == 0    where depth > 0: depth = clip(depth + std n, 0, FLT_MAX).  depth > 0 is false for NaN:
 *                    NaN stays, and so do 0 and negative values (the reference's np.clip would raise a negative one to 0).
 *   hp_aug_depth_noise, correlated != 0    a grid of d_grid_h[b] x d_grid_w[b] cells (the host's int(h / f), int(w / f)), cell c =
 *                    std n(c), is upsampled to h x w bicubically as OpenCV documents INTER_CUBIC: for output x,
 *                    fx = (x + 0.5)(gw / w) - 0.5, sx = floor(fx), t = fx - sx, taps sx - 1 .. sx + 2 clamped to the grid with
 *                      w0 = ((A (t + 1) - 5 A)(t + 1) + 8 A)(t + 1) - 4 A,  w1 = ((A + 2) t - (A + 3)) t t + 1,
 *                      w2 = ((A + 2)(1 - t) - (A + 3))(1 - t)(1 - t) + 1,   w3 = 1 - w0 - w1 - w2,   A = -0.75,
 *                    the same along y; value = sum_j wy_j (sum_i wx_i g[y_j][x_i]), both sums from tap 0 onto 0, in float32.
 *                    It is added where depth > 0 and the sum clipped as above.  A grid with a side <= 0 (or more cells than
 *                    pixels) leaves the image unchanged.
 *   hp_aug_depth_missing   of the n_valid pixels with depth > 0 exactly m = (int)(d_fraction[b] * n_valid) (double; at most n_valid)
 *                    become 0: the m with the smallest (r0, pixel index) pairs, r0 from stream _MISSING.  One workgroup per
 *                    image: the words go to the workspace, then a radix select, 8 bits a pass with an integer histogram in the
 *                    LDS, finds the m-th smallest 64-bit key (r0 << 32 | pixel).  No sort, no host round trip.  n_valid == 0 or
 *                    m == 0 leaves the image unchanged.
 *   hp_aug_depth_ellipses  d_table [B][max_ellipses][5] float32 = (u, rx, ry, angle_deg, value), d_count [B] int32 (clamped to
 *                    0 .. max_ellipses).  The centre (cx, cy) of ellipse e is the floor(u n_valid)-th (double; clamped to
 *                    n_valid - 1) valid pixel in row-major order, found on the device by a prefix count over groups of 64 pixels.
 *                    rx, ry are the radii the host has rounded to integers.  With dx = x - cx, dy = y - cy,
 *                    th = angle_deg * 0.017453292f:  x' = dx cos th + dy sin th,  y' = dy cos th - dx sin th, a pixel is inside when
 *                    (x' / max(rx, 0.5))^2 + (y' / max(ry, 0.5))^2 <= 1  in float32.  noise == 0: inside pixels become 0.
 *                    noise != 0: where depth > 0, depth += the value of the LAST ellipse in table order that covers the pixel
 *                    (no clip, as in the reference).  n_valid == 0 leaves the image unchanged -- the reference raises there.
 *                    OpenCV fills a polygon approximation of the ellipse: boundary pixels may differ (unpinned).
 *   hp_aug_depth_blur      the k x k normalised box filter, k = d_ksize[b], border reflect-101, anchor k / 2 (integer division:
 *                    k = 4 covers x - 2 .. x + 1): the k k values are added in float32 onto 0, rows from the top, each row from
 *                    the left, and the sum divided by (float)(k k).  Zeros take part, as in the reference.  k_max is the HOST's
 *                    bound on d_ksize: k_max > h or k_max > w is HP_ERR_ARG (reflect-101 is not defined) and launches nothing; an
 *                    image whose k is outside 1 .. k_max is left unchanged.
 *   hp_aug_depth_mask      d_segmentation == NULL: depth = 0 (DepthDropout); else depth = 0 where segmentation == 0.
 * ---------------------------------------------------------------------------------- */
#define HP_AUG_OP_BRIGHTNESS 0
#define HP_AUG_OP_COLOR 1
#define HP_AUG_OP_CONTRAST 2
#define HP_AUG_OP_SHARPNESS 3
#define HP_AUG_STREAM_NOISE 1
#define HP_AUG_STREAM_GRID 2
#define HP_AUG_STREAM_MISSING 3
int64_t hp_aug_workspace_bytes(int B, int h, int w, int max_ellipses);
int hp_aug_rgb_enhance(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_op, const float* d_factor, const uint8_t* d_apply,
                       uint8_t* d_out, void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_aug_rgb_blur(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_radius, const uint32_t* d_ww, const uint32_t* d_fw,
                    const uint8_t* d_apply, uint8_t* d_out, int force_general, void* d_workspace, int64_t workspace_bytes,
                    void* stream);
int hp_aug_replace_background(int B, int h, int w, const uint8_t* d_rgb, const int32_t* d_segmentation, const uint8_t* d_background,
                              const uint8_t* d_apply, uint8_t* d_out, void* stream);
int hp_aug_depth_noise(int B, int h, int w, const float* d_depth, const float* d_std, int correlated, const int32_t* d_grid_h,
                       const int32_t* d_grid_w, const uint8_t* d_apply, uint64_t seed, float* d_out, void* d_workspace,
                       int64_t workspace_bytes, void* stream);
int hp_aug_depth_missing(int B, int h, int w, const float* d_depth, const double* d_fraction, const uint8_t* d_apply, uint64_t seed,
                         float* d_out, void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_aug_depth_ellipses(int B, int h, int w, const float* d_depth, const float* d_table, const int32_t* d_count, int max_ellipses,
                          int noise, const uint8_t* d_apply, float* d_out, void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_aug_depth_blur(int B, int h, int w, const float* d_depth, const int32_t* d_ksize, int k_max, const uint8_t* d_apply,
                      float* d_out, void* stream);
int hp_aug_depth_mask(int B, int h, int w, const float* d_depth, const int32_t* d_segmentation, const uint8_t* d_apply, float* d_out,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * Frame geometry: Pillow-exact resize of a batch of frames that already lives on the device, and modal boxes from an id map --
 * what the reference's CropResizeToAspectTransform and ReplaceBackgroundTransform do with PIL.Image.crop / resize and
 * make_detections_from_segmentation.  csrc/resize.hip; the user-facing layer is happypose_amd/augmentations.py.
 *
 * All images of a call share the input size, the output size and the filter.  The geometry of image b -- its crop rectangle and its
 * source box -- is in TABLE SET d_table_of[b] (0 .. n_tables - 1; another value leaves the image's output untouched): the host
 * computes the tables (happypose_amd.ops.resize_tables, float64), so the box may differ per image exactly when the images name
 * different table sets, and images with the same geometry share one.  There is therefore no box argument: the tables hold SOURCE
 * pixel indices.  A tap or an index outside the frame reads 0 -- that is PIL.Image.crop's padding when a crop rectangle leaves the
 * frame -- and the kernels clamp every count to the table's width, so no table content can make them touch memory outside the
 * buffers they were given.  d_apply [B] uint8: the OUTPUT of an image with d_apply[b] == 0 is not written (it keeps what d_out
 * held).  d_out must not alias d_in.  B == 0 returns HP_OK and launches nothing; a null pointer, a size <= 0, B > 65535, more than
 * 2^28 pixels per image or out_h > 65535 is HP_ERR_ARG before the GPU is touched.  Integer arithmetic and copies only: results are
 * bit-identical from run to run and do not depend on the other images.
 *
 * hp_resize_rgb     Image.resize(size, BILINEAR | BICUBIC, box) of 8-bit RGB, d_in [B][in_h][in_w][3] -> d_out [B][out_h][out_w][3]
 *                   (pinned against Pillow 12.2 by tests/golden/g15_resize.npz).  Per axis, with in = the (cropped) image's size,
 *                   box = (b0, b1) and out the output size, in double:  scale = (b1 - b0) / out, fscale = max(scale, 1),
 *                   support = S fscale (S = 1 bilinear, 2 bicubic); for output index i: centre = b0 + (i + 0.5) scale,
 *                   lo = max((int)(centre - support + 0.5), 0), hi = min((int)(centre + support + 0.5), in); the weight of source j
 *                   in [lo, hi) is f((j - centre + 0.5) / fscale), f the triangle or the cubic with a = -0.5, divided by the
 *                   window's sum, then rounded to fixed point: (int)(w 2^22 + 0.5), (int)(w 2^22 - 0.5) below zero.
 *                     d_xbounds [n_tables][out_w][2] = (lo + the crop's origin, hi - lo),  d_xweights [n_tables][out_w][ksize_x]
 *                   and the same along y.  A pass is  out = clip((2^21 + sum_k weights[i][k] in[lo + k]) >> 22, 0, 255)  in 32-bit
 *                   signed integers (arithmetic shift).  The pass along x runs first into a uint8 intermediate
 *                   [B][in_h][out_w][3] in d_workspace (only the rows the pass along y reads), then the pass along y.  Pillow
 *                   skips a pass whose axis keeps its size with the whole axis as box; the host says so with ksize_x == 0
 *                   (then out_w == in_w) or ksize_y == 0 (then out_h == in_h), the tables of a skipped pass may be NULL, and a
 *                   call with both skipped copies the frames.  (A skipped pass would be the identity: its weights are 2^22 on
 *                   one tap.)  band_x: the host's bound on the source pixels one tile of 256 consecutive output pixels covers,
 *                   max over tiles and table sets of (lo + n of the tile's last index) - (lo of its first); the pass along x
 *                   stages that band in the LDS.  band_x > 12288, or a ksize > 4096, is HP_ERR_ARG and launches nothing; a band
 *                   smaller than the tables need is not an overrun, the taps beyond it read 0.
 *                   d_workspace: hp_resize_workspace_bytes(B, in_h, out_w) = roundup8(3 B in_h out_w) bytes (-1 for sizes out of
 *                   range), needed only when both passes run.
 * hp_resize_nearest Image.resize(size, NEAREST, box) of modes I and F: d_in / d_out are 4-byte pixels copied as bits (NaN, negative
 *                   depths and negative ids pass through).  d_xindex [n_tables][out_w], d_yindex [n_tables][out_h]: the source
 *                   index of every output index, (int) t_i with t_0 = b0 + scale / 2 and t_{i + 1} = t_i + scale -- a RUNNING sum in
 *                   double, as Pillow tabulates it -- plus the crop's origin; an index outside the frame (-1 included) gives 0.
 * hp_seg_boxes      d_segmentation [B][h][w] int32, d_ids [B][max_ids] int32, d_count [B] (clamped to 0 .. max_ids), 1 <= max_ids
 *                   <= 256.  d_boxes [B][max_ids][4] int32 = (x1, y1, x2, y2), the INCLUSIVE min and max of the columns and rows
 *                   where segmentation == ids[b][k], as the reference's make_detections_from_segmentation; d_n_px [B][max_ids] the
 *                   number of such pixels.  A slot whose id is absent, or at or above d_count[b], has n_px 0 and an unspecified
 *                   box.  An id listed twice is counted in its first slot.  Integer min / max / add reductions in the LDS per
 *                   workgroup, then integer atomics on the table: exact whatever the order.
 * ---------------------------------------------------------------------------------- */
int64_t hp_resize_workspace_bytes(int B, int in_h, int out_w);
int hp_resize_rgb(int B, int in_h, int in_w, int out_h, int out_w, const uint8_t* d_in, int n_tables, const int32_t* d_table_of,
                  const int32_t* d_xbounds, const int32_t* d_xweights, int ksize_x, int band_x, const int32_t* d_ybounds,
                  const int32_t* d_yweights, int ksize_y, const uint8_t* d_apply, uint8_t* d_out, void* d_workspace,
                  int64_t workspace_bytes, void* stream);
int hp_resize_nearest(int B, int in_h, int in_w, int out_h, int out_w, const void* d_in, int n_tables, const int32_t* d_table_of,
                      const int32_t* d_xindex, const int32_t* d_yindex, const uint8_t* d_apply, void* d_out, void* stream);
int hp_seg_boxes(int B, int h, int w, const int32_t* d_segmentation, const int32_t* d_ids, const int32_t* d_count, int max_ids,
                 int32_t* d_boxes, int32_t* d_n_px, void* stream);

/* ------------------------------------------------------------------------------------
 * Hypothesis generation of the trainers' forward-loss step (csrc/train_hyp.hip; the user-facing layer is
 * happypose_amd/training.py).  Replaces add_noise (TB/lib3d/transform_ops.py:70-104 == CP/lib3d/transform_ops.py, a host loop over
 * transforms3d.euler.euler2mat) and TCO_init_from_boxes (TB/lib3d/cosypose_ops.py:159-181 == CP/lib3d/cosypose_ops.py:146-168).
 * One thread per output row, no atomics: a row is a function of its own inputs and bit-identical from run to run.
 *
 * hp_pose_add_noise       d_TCO [n / repeat][4][4], d_TCO_out [n][4][4]: output row i is a noisy copy of pose i / repeat (repeat >= 1
 *                         divides n: the n_hypotheses copies per image are made inside the launch).  d_TCO_out may be d_TCO itself
 *                         when repeat == 1; any other overlap is HP_ERR_ARG.
 *  Noise, given           d_noise_in [n][6] float32 = (ai, aj, ak) in RADIANS, (dx, dy, dz) in metres, used as they are;
 *                         euler_deg_std / trans_std (HOST arrays of 3) and seed / row_offset are then not read.
 *  Noise, drawn           d_noise_in == NULL.  row = row_offset + i (64 bits); Philox4x32-10 (constants as for
 *                         hp_mesh_sample_surface) with key (seed & 0xffffffff, seed >> 32) and the two counters
 *                         (row & 0xffffffff, row >> 32, j, 0), j = 0, 1, giving the words w[4 j + 0 .. 3].  Pair p = 0, 1, 2:
 *                           u1 = ((w[2 p] >> 8) + 1) 2^-24 in (0, 1],  u2 = (w[2 p + 1] >> 8) 2^-24 in [0, 1)
 *                           z[2 p] = sqrt(-2 ln u1) cos(2 pi u2),  z[2 p + 1] = sqrt(-2 ln u1) sin(2 pi u2)
 *                         (w[6], w[7] unused) and  noise[k] = z[k] euler_deg_std[k] pi / 180,  noise[3 + k] = z[3 + k] trans_std[k],
 *                         k = 0, 1, 2, evaluated in double and rounded once to float32.  Those six floats go to d_noise_out [n][6]
 *                         (may be NULL; also written, as a copy, when the noise is given) and into the pose, so a second call with
 *                         them as d_noise_in gives the same bits.  A row depends on (seed, row_offset + i) and its pose, not on n.
 *                         A negative or NaN standard deviation is HP_ERR_ARG.
 *  Pose                   R_noise = euler2mat(ai, aj, ak), static axes xyz ('sxyz'): Rz(ak) Ry(aj) Rx(ai), i.e.
 *                           [ cy cz   sx sy cz - cx sz   cx sy cz + sx sz ]
 *                           [ cy sz   sx sy sz + cx cz   cx sy sz - sx cz ]
 *                           [ -sy     sx cy              cx cy            ]
 *                         R_out = R R_noise (double from the float32 inputs, each entry rounded once), t_out = t + dt (float32),
 *                         bottom row copied.  ai == aj == ak == 0 leaves the 3 x 3 block, and dt[k] == 0 leaves t[k], bit for bit:
 *                         a standard deviation of 0 switches that part of the noise off exactly.
 * hp_tco_init_from_boxes  row i: box d_boxes[d_box_ids ? d_box_ids[i] : i] = (x1, y1, x2, y2) of d_boxes [n_boxes][4], intrinsics
 *                         d_K[d_im_ids ? d_im_ids[i] : i] of d_K [n_images][9];  z = (z_lo + z_hi) / 2,
 *                         t = (((x1 + x2) / 2 - cx) z / fx, ((y1 + y2) / 2 - cy) z / fy, z) in float32 in that order of
 *                         operations, identity rotation.  An id outside its table gives a NaN pose and reads nothing outside
 *                         the tables, see hp_pose_prep.
 * n == 0 returns HP_OK and launches nothing.
 * ---------------------------------------------------------------------------------- */
int hp_pose_add_noise(int n, int repeat, const float* d_TCO, const float* euler_deg_std /* host [3] */,
                      const float* trans_std /* host [3] */, uint64_t seed, uint64_t row_offset, const float* d_noise_in,
                      float* d_TCO_out, float* d_noise_out, void* stream);
int hp_tco_init_from_boxes(int n, const float* d_boxes, int n_boxes, const int32_t* d_box_ids, const float* d_K, int n_images,
                           const int32_t* d_im_ids, float z_lo, float z_hi, float* d_TCO_out, void* stream);

/* ------------------------------------------------------------------------------------
 * The candidate views and the hypothesis draw of the coarse classifier's training step (csrc/train_hyp.hip):
 * make_TCO_multiview(TCO, tCR, "sphere_26views", remove_TCO_rendering=True, views_inplane_rotations=True)
 * (TB/lib3d/multiview.py:153-163, 224-251) and the per-image np.random.permutation / rand / randint of
 * MP/training/megapose_forward_loss.py:126-141, which the reference runs on the host with Panda3D node paths.
 *
 * Candidates.  Pose d_TCO [b][16] (row-major 4 x 4), reference point d_tCR [b][3] in camera 0 (NULL: the pose's translation).
 * The 26 views are cameras at  |tCR| (x, y, z)  in the Panda frame (x right, y forward, z up) of camera 0 re-aimed at tCR,
 * (x, y, z) in the reference's loop order: y in (0, 1, 2) outermost, x in (0, -1, 1), z in (0, 1, -1) innermost, without (0, 1, 0)
 * -- view 0 is (0, 0, 0), view 1 (0, 0, 1), ... view 9 (0, 1, 1) ... view 25 (1, 2, -1).  Each looks at tCR with camera 0's up as
 * the hint: forward f exact, right = f x up / |f x up|, up' = right x f, evaluated in double in camera-0 OpenCV axes exactly as
 * hp_pose_prep evaluates its front views (one shared device function); then TCV_O = invert_transform_matrices(TC0_CV) @ TCO in
 * float32.  A pose with a non-finite entry in its upper 3 x 4 (or a non-finite d_tCR row), and |tCR| == 0, take the identity
 * view, the rule of hp_pose_prep.
 *   Degenerate look-at: where |f x up| < 1e-9 (f and up unit vectors) the hint defines no right vector and right is the right
 *   axis of the re-aimed camera 0.  Offsets (0, 1, +-1) meet this when tCR_y is exactly 0; Panda3D's answer there is not
 *   reproduced (like lookAt itself this is this library's definition, UNPINNED against the reference).
 * In-plane rotations: candidate index = view * 4 + rot, rot = 0 .. 3; the rotation block is Rz(rot pi / 2) R with the exact
 * entries 0 / +-1 (rot 1: rows (-r1, r0, r2); rot 2: (-r0, -r1, r2); rot 3: (r1, -r0, r2)), the translation is the view's.
 * Candidate 0 is camera 0 re-aimed at the object without in-plane rotation: the classifier's positive.
 * hp_views_sphere26 writes d_TCV_O [b][104][16], or [b][26][16] with inplane_rotations == 0 (bit for bit every fourth candidate).
 *
 * hp_coarse_hypotheses draws n_hyp (1 .. 104) of the 104 candidates per image and evaluates only those: d_hyp [b][n_hyp][16],
 * d_view_ids [b][n_hyp] int32, d_is_positive [b][n_hyp] float32 (1 where the id is 0).  Image i draws from (seed, row_offset + i)
 * alone: row = row_offset + i (64 bits), Philox4x32-10 (constants as for hp_mesh_sample_surface) with key
 * (seed & 0xffffffff, seed >> 32) and counters (row & 0xffffffff, row >> 32, j, 0), j = 0 .. 26, giving words w[4 j + 0 .. 3].
 *   ids     perm = (0, 1, .. 103); for i = 0 .. n_hyp - 1:  k = i + floor(w[i] (104 - i) / 2^32), swap perm[i], perm[k]
 *           (integer arithmetic; the first n_hyp entries of a uniform random permutation).  Bias: k takes each of its 104 - i
 *           values for floor or ceil of 2^32 / (104 - i) words, so its probability differs from 1 / (104 - i) by less than 2^-32
 *           (relative: less than 104 x 2^-32 = 2.5e-8).
 *   forced  where id 0 is absent and  w[104] > floor((1 - p_force_positive) 2^32)  (1 - p in binary64; u = w 2^-32 > 0.3 for the
 *           reference's p = 0.7), slot floor(w[105] n_rendered_views / 2^32) becomes id 0: the reference's
 *           randint(cfg.n_rendered_views), slot 0 for its one rendered view.  1 <= n_rendered_views <= n_hyp.
 * The reference's global np.random stream is not reproduced.  No atomics: outputs are bit-identical from run to run, and
 * d_hyp[i][h] holds the bits hp_views_sphere26 gives for candidate d_view_ids[i][h].  b == 0 returns HP_OK and launches nothing.
 * ---------------------------------------------------------------------------------- */
#define HP_SPHERE26_VIEWS 26
#define HP_SPHERE26_CANDIDATES 104
int hp_views_sphere26(int b, const float* d_TCO, const float* d_tCR /* [b][3] or NULL */, int inplane_rotations, float* d_TCV_O,
                      void* stream);
int hp_coarse_hypotheses(int b, int n_hyp, int n_rendered_views, double p_force_positive, const float* d_TCO, uint64_t seed,
                         uint64_t row_offset, float* d_hyp, int32_t* d_view_ids, float* d_is_positive, void* stream);

/* ------------------------------------------------------------------------------------
 * The detector's training targets and losses (csrc/det_losses.hip; the user-facing layer is happypose_amd/detection_losses.py and
 * happypose_amd.training.h_maskrcnn).  What torchvision 0.14's train-mode MaskRCNN.forward computes between the networks:
 * models/detection/rpn.py, roi_heads.py, _utils.py (Matcher, BalancedPositiveNegativeSampler, BoxCoder), ops/boxes.py,
 * ops/roi_align.py.  torchvision cannot be run beside this library: parity with it is UNPINNED, the definitions below are the
 * contract and tests/det_losses_ref.py restates them in float64.
 *
 * Rows are the boxes of a whole batch: d_image_of [n] int32 names each row's image (0 .. n_images - 1), the ground truths of all
 * images are one table d_gt [n_gt][4] (x1, y1, x2, y2) and image b owns rows d_gt_off[b] .. d_gt_off[b + 1] - 1 of it
 * (d_gt_off [n_images + 1], ascending from 0 to n_gt).  Ground-truth indices (d_match) are indices into that table.
 * Every entry point returns HP_OK and launches nothing when its row count is 0, and HP_ERR_ARG for a negative size, a null
 * pointer or a workspace that is too small.  No floating-point atomics: sums run per lane in row order, over the wavefront by
 * shuffles, over the wavefronts in LDS, and over the workgroups' partials in a second launch, so two calls give the same bits and
 * a row's targets and gradient do not depend on the other rows.  The host layer range-checks every index column before a launch;
 * the kernels answer an index outside its table with NaN (or background) and touch nothing outside the tables.
 *
 * hp_det_assign        Matcher(high, low, allow_low_quality) on box_iou(gt of the row's image, boxes).  IoU in float32 by one
 *                      device function used by both passes (no contraction): area = (x2 - x1)(y2 - y1) of both, lt = max, rb =
 *                      min, wh = max(rb - lt, 0), inter = w h, iou = inter / ((a1 + a2) - inter).
 *                      Pass 1: per ground truth the maximum IoU over the boxes of its image (partials in d_workspace,
 *                      hp_det_assign_workspace_bytes(n, n_gt) bytes; -1 for negative sizes).  Pass 2: per box the FIRST maximum in
 *                      ground-truth order (d_iou [n], its IoU); d_match [n] = that ground truth, -1 where the IoU < low, -2 where
 *                      low <= IoU < high.  allow_low_quality != 0: set_low_quality_matches_ -- every box whose IoU with ANY
 *                      ground truth of its image EQUALS (float ==, ties included) that ground truth's maximum gets its
 *                      pre-threshold match back.  An image without ground truths gives -1 and IoU 0 in every row.
 *                      n_gt <= 65535; low <= high.
 * hp_det_sample_keys   the seeded half of BalancedPositiveNegativeSampler: d_keys[i] = word 0 of Philox4x32-10 (constants as for
 *                      hp_mesh_sample_surface) with key (seed & 0xffffffff, seed >> 32) and counter (d_index_in_image[i],
 *                      d_image_of[i], stream_id, 0).  The selection (the k rows with the smallest (key, index) per image and
 *                      class) is the host layer's; torch's randperm stream is not reproduced.
 * hp_det_box_encode    BoxCoder.encode_single with weights (wx, wy, ww, wh): reference box d_gt[d_match[i]], the zero box where
 *                      d_match[i] is outside 0 .. n_gt - 1; proposal d_boxes[i].  float32, torchvision's order:
 *                      ex_w = px2 - px1, ex_cx = px1 + 0.5 ex_w, gt_w, gt_cx likewise; dx = wx (gt_cx - ex_cx) / ex_w,
 *                      dw = ww log(gt_w / ex_w); d_out [n][4] = (dx, dy, dw, dh).
 * hp_det_mask_targets  project_masks_on_boxes: roi_align(d_masks[d_match[i]], d_rois[i], (M, M), spatial_scale 1, sampling_ratio
 *                      -1, aligned False).  d_masks [n_gt][h][w] uint8 (its values as floats), d_out [n][M][M] float32.  float32, in
 *                      the order of torchvision's kernel: roi_w = max(x2 - x1, 1), bin = roi_w / M, grid = ceil(roi_w / M)
 *                      samples per bin and axis at x1 + pw bin + (ix + 0.5) bin / grid, bilinear taps (0 outside [-1, size],
 *                      clamped at the borders), summed over iy then ix, divided by the number of samples.  One workgroup per roi.
 *                      An index outside the table, or a roi that is not finite, gives NaN.
 * The three losses write the loss and, for an upstream gradient of 1, the gradient with respect to the network's output in the
 * same pass (the normalisers are known before the launch).  Every term is evaluated in double from the float32 inputs and
 * accumulated in double; log(1 + exp(-|x|)) is log1p(exp(-|x|)).  A non-finite input in a row makes the loss, and that row's
 * gradient, NaN.  d_workspace: hp_det_loss_workspace_bytes(rows) bytes with rows = ceil(n_sampled / 256), ceil(n / 256) or n.
 * hp_loss_rpn          d_sampled [n_sampled] int32: distinct anchor indices.  d_labels [n_anchors] int32 (>= 1 positive, 0
 *                      negative).  d_loss[0] = mean over the sampled rows of binary_cross_entropy_with_logits(objectness, label >=
 *                      1); d_loss[1] = sum over the sampled positives of smooth_l1(deltas - targets, beta = 1/9) / n_sampled.
 *                      d_grad_objectness [n_anchors], d_grad_deltas [n_anchors][4]: zeroed by the call, then the sampled rows.
 * hp_loss_fastrcnn     d_class_logits [n][ld], n_classes <= ld (columns beyond n_classes are not read; their gradient is 0),
 *                      d_box_regression [n][ld_reg] (4 n_classes <= ld_reg), d_labels [n] int32 in 0 .. n_classes - 1,
 *                      d_targets [n][4].  d_loss[0] = mean softmax cross-entropy (row maximum subtracted); d_loss[1] = sum of
 *                      smooth_l1(beta = 1/9) over the four values of the row's own class for rows with label > 0, / n.
 * hp_loss_mask         d_mask_logits [n][n_classes][M][M], d_targets [n][M][M]: d_loss[0] = mean over n M M of
 *                      binary_cross_entropy_with_logits(logits[i][label_i], target_i); the gradient is 0 outside the label's
 *                      channel.  n == 0 launches nothing (the host layer returns a loss of 0).
 * ---------------------------------------------------------------------------------- */
int64_t hp_det_assign_workspace_bytes(int n, int n_gt);
int hp_det_assign(int n, const float* d_boxes, const int32_t* d_image_of, int n_images, const float* d_gt, int n_gt,
                  const int32_t* d_gt_off, float high, float low, int allow_low_quality, int32_t* d_match, float* d_iou,
                  void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_det_sample_keys(int n, const int32_t* d_index_in_image, const int32_t* d_image_of, uint32_t stream_id, uint64_t seed,
                       uint32_t* d_keys, void* stream);
int hp_det_box_encode(int n, const float* d_boxes, const int32_t* d_match, const float* d_gt, int n_gt, float wx, float wy, float ww,
                      float wh, float* d_out, void* stream);
int hp_det_mask_targets(int n, const uint8_t* d_masks, int n_gt, int h, int w, const int32_t* d_match, const float* d_rois, int m,
                        float* d_out, void* stream);
int64_t hp_det_loss_workspace_bytes(int n_rows);
int hp_loss_rpn(int n_anchors, int n_sampled, const int32_t* d_sampled, const float* d_objectness, const float* d_deltas,
                const int32_t* d_labels, const float* d_targets, float* d_loss, float* d_grad_objectness, float* d_grad_deltas,
                void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_loss_fastrcnn(int n, int n_classes, int ld, int ld_reg, const float* d_class_logits, const float* d_box_regression,
                     const int32_t* d_labels, const float* d_targets, float* d_loss, float* d_grad_logits, float* d_grad_regression,
                     void* d_workspace, int64_t workspace_bytes, void* stream);
int hp_loss_mask(int n, int n_classes, int m, const float* d_mask_logits, const int32_t* d_labels, const float* d_targets, float* d_loss,
                 float* d_grad_logits, void* d_workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Batch assembly of the training data sets: the step between a scene observation and the trainers' steps -- the reference's
 * PoseDataset.make_data_from_obs + collate_fn (toolbox/datasets/pose_dataset.py) and DetectionDataset.make_data_from_obs
 * (cosypose/datasets/detection_dataset.py) -- on frames, id maps and box tables that already live on the device.
 * csrc/batch_data.hip; the user-facing layer is happypose_amd/datasets.py.
 *
 * Integers and copied bits only, except the pose product of hp_pose_batch_select; no atomics, one writer per output element:
 * results are bit-identical from run to run.  Counts and indices read from device memory (d_count, d_dst, d_slot_row) are checked
 * against the tables they address: a value outside is clamped or skipped, never followed.  B == 0 returns HP_OK and launches
 * nothing; a null pointer, max_ids outside 1 .. 256, B > 65535 (gather, masks), a side < 1 or more than 2^28 pixels per frame is
 * HP_ERR_ARG before the GPU is touched.
 *
 * hp_pose_batch_select  one object per frame.  d_n_px [B][max_ids] and d_boxes [B][max_ids][4] int32 as hp_seg_boxes writes them
 *                   (inclusive x1, y1, x2, y2), d_count [B] (clamped to 0 .. max_ids), d_keep [B][max_ids] uint8 or NULL (the host
 *                   evaluates keep_labels_set into it), d_TWC [B][4][4], d_TWO [B][max_ids][4][4] float32, row-major.
 *                   Slot k of frame b is VALID when
 *                     n_px > 0                                   remove_invisible_objects and `unique_id in unique_ids_visible`
 *                                                                (the reference's second condition, `np.all(obj.bbox_modal) >= 0`,
 *                                                                compares a boolean with 0 and is always true as written; it is not
 *                                                                "fixed" here: there is no such condition)
 *                     (x2 - x1) (y2 - y1) >= min_area            when min_area >= 0 (negative: no such condition; NaN: HP_ERR_ARG):
 *                                                                the reference's arithmetic on the INCLUSIVE box, without + 1, so a
 *                                                                one-pixel object has area 0; the product is an integer, compared
 *                                                                in double
 *                     d_keep[b][k] != 0                          when d_keep is given.
 *                   The chosen slot is the first valid one (first != 0: return_first_object) or the k-th valid one in slot order,
 *                   k = mulhi32(x0, n_valid) = (x0 n_valid) >> 32, x0 = word 0 of Philox4x32-10 with key (seed lo, seed hi) and
 *                   counter (row lo, row hi, 0, 0), row = row_offset + b in 64 bits -- the constants and the key layout of
 *                   hp_pose_add_noise, so a frame's choice depends on (seed, row_offset + b) and its own table alone.  The
 *                   reference's random.sample stream is not reproduced.
 *                   d_chosen [B] int32 (-1: no valid slot), d_valid [B] uint8, d_bbox [B][4] float32 the chosen box,
 *                   d_TCO [B][4][4] = inverse(TWC) @ TWO[chosen] with the RIGID inverse: Ti[i][k] = TWC[k][i] (k < 3),
 *                   Ti[i][3] = -((TWC[0][i] t0 + TWC[1][i] t1) + TWC[2][i] t2), t = TWC[.][3];
 *                   TCO[i][j] = ((Ti[i][0] B[0][j] + Ti[i][1] B[1][j]) + Ti[i][2] B[2][j]) + Ti[i][3] B[3][j] for i < 3, evaluated in
 *                   double from the float32 inputs in this order and rounded once; row 3 is TWO's row 3, copied.  A frame without a
 *                   valid slot has bbox and TCO 0.  d_dst [B] int32: the exclusive scan of d_valid, the row of frame b among the
 *                   valid frames (defined for every b); d_n_valid [1] their number (0 when B == 0).
 * hp_batch_gather_chw   the collate step.  d_rgb [B][h][w][3] uint8 -> d_out_rgb [n_out][3][h][w]: frame b goes to row d_dst[b]; a
 *                   frame with d_valid[b] == 0 or a row outside 0 .. n_out - 1 is skipped, and rows no frame names keep what they
 *                   held.  With d_depth [B][h][w] float32 (and d_out_depth [n_out][h][w]; both or neither) the depth follows in the
 *                   same launch, bits copied (NaN, -0).  Loads and stores are 16-byte vectors on the 16-byte grid of each address,
 *                   the interleaved-to-planar transposition goes through the LDS, and byte ranges that do not start or end on the
 *                   grid (h w odd) are completed byte by byte by the lanes that own the straddling vectors.  The outputs must not
 *                   alias the inputs.
 * hp_instance_masks     the detector's targets.  d_segmentation [B][h][w] int32, d_ids [B][max_ids], d_count [B] as for
 *                   hp_seg_boxes; d_slot_row [B][max_ids] int32: the output row of a kept slot, -1 (or any value outside
 *                   0 .. G - 1) for a slot that is not kept; the rows of kept slots are distinct.  d_masks [G][h][w] uint8:
 *                   masks[row] = (segmentation[b] == ids[b][slot]), 0 / 1.  A frame's id map is read once and all of its masks are
 *                   written from it, 16 pixels per vector store.  Rows are written completely: the caller need not clear d_masks.
 *                   G == 0 and frames without kept slots are legal.
 * ---------------------------------------------------------------------------------- */
int hp_pose_batch_select(int B, int max_ids, const int32_t* d_n_px, const int32_t* d_boxes, const int32_t* d_count, const uint8_t* d_keep,
                         float min_area, int first, uint64_t seed, uint64_t row_offset, const float* d_TWC, const float* d_TWO,
                         int32_t* d_chosen, uint8_t* d_valid, float* d_bbox, float* d_TCO, int32_t* d_dst, int32_t* d_n_valid, void* stream);
int hp_batch_gather_chw(int B, int h, int w, const uint8_t* d_rgb, const float* d_depth, const uint8_t* d_valid, const int32_t* d_dst,
                        int n_out, uint8_t* d_out_rgb, float* d_out_depth, void* stream);
int hp_instance_masks(int B, int h, int w, const int32_t* d_segmentation, const int32_t* d_ids, const int32_t* d_count,
                      const int32_t* d_slot_row, int max_ids, int G, uint8_t* d_masks, void* stream);

/* ------------------------------------------------------------------------------------
 * Training the linear heads on a frozen backbone (csrc/head_train.hip; the user-facing layer is happypose_amd.training.HeadTrainer).
 * The heads are the ones csrc/pool_head.hip evaluates: out[b][o] = W[o] . feat[b] + bias[o], rows o = 0 .. pose_dim - 1 the pose
 * head and pose_dim .. O - 1 the rendered-view logits (O = pose_dim + n_logits <= 32), feat [B][C] the spatial mean or, on the
 * torchvision-ResNet path, the output of the 512 x 512 fc (the features output of hp_net_forward).  The optimiser is the one the
 * reference's trainers construct (CP/training/train_pose.py:374-378, MP/training/utils.py:115-135: torch.optim.Adam), its clipping
 * torch.nn.utils.clip_grad_norm_ (train_pose.py:438-442, MP/training/train_megapose.py:360-363).  All fp32.  No floating-point
 * atomics: every sum has one order that depends on the sizes alone -- results are bit-identical from run to run and independent of
 * the launch grid.  u = 2^-24 below.
 *
 * hp_head_backward    g[b][o] = w[b] d_out[b][o], rounded once (d_w == NULL: g = d_out, no product); d_out is given in two parts,
 *                     d_pose_grad [B][pose_dim] and d_logit_grad [B][n_logits], and a NULL d_logit_grad stands for zeros.
 *                       dW[o][c]     = sum_b g[b][o] feat[b][c]         [O][C]
 *                       db[o]        = sum_b g[b][o]                    [O]
 *                       d_dfeat[b][c] = sum_o g[b][o] W[o][c]           [B][C], optional (NULL: not computed; it needs d_W [O][C]):
 *                                                                        what hp_fc_backward, and later a backbone's backward, reads
 *                     Order of the sum over b: rows are cut into chunks of 64 in index order (chunk k = rows 64 k .. 64 k + 63);
 *                     inside a chunk acc = fma(g, feat, acc) from acc = 0 in row order (db: plain additions); the chunks' partial
 *                     sums are added in index order, s = p_0, s += p_k; with accumulate != 0 the result is then ADDED to what
 *                     dW / db hold (dW = dW + s), else it replaces it.  A term meets at most B + 2 roundings, so
 *                     |dW - exact| <= (B + 2) u sum_b |g feat| per element.  d_dfeat is an fma chain over o = 0 .. O - 1 from 0.
 *                     d_ws: hp_head_backward_ws_floats(B, C, O) = ceil(B / 64) (O C + O) floats.  B == 0: zeros (or nothing added).
 * hp_fc_backward      the same reduction for a layer with many outputs, dW[o][c] = sum_b d_dout[b][o] d_in[b][c] ([O][C];
 *                     the fc: O = C = 512, d_dout the d_dfeat above, d_in the pooled input of hp_net_set_pooled_out) and
 *                     db[o] = sum_b d_dout[b][o].  Here the outputs supply the parallelism and the sum over b is ONE chain in row
 *                     order per element, acc = fma(d_dout, d_in, acc) from 0 (db: plain additions); accumulate as above.
 * hp_grad_sq_norm     d_sq_norm[0] = sum_i g[i]^2 over a flat buffer, N <= 2^31 - 1.  Two levels: workgroup k of 256 lanes takes
 *                     elements 1024 k .. 1024 k + 1023, lane t the four x_j = g[1024 k + t + 256 j] (0 past N) as
 *                     (x0 x0 + x1 x1) + (x2 x2 + x3 x3); the 64 lanes of a wavefront meet in a butterfly (partner lane ^ 1, ^ 2,
 *                     .. ^ 32), the four wavefronts as (s0 + s1) + (s2 + s3).  With more than one workgroup a second launch of ONE
 *                     workgroup adds the partials: lane t takes t, t + 256, ... in index order, then the same butterfly and wave
 *                     sum.  d_ws: hp_grad_sq_norm_ws_floats(N) = ceil(N / 1024) floats (not read when that is 1).
 * hp_adamw_step       one launch over p, g, m, v [N]; g is not written.  step counts from 1.  With d_sq_norm and d_max_norm (device
 *                     scalars, both or neither) the gradient is first clipped as clip_grad_norm_ does, inside the launch -- no host
 *                     read-back between the backward and the step:
 *                       g = g min(max_norm / (sqrt(sq_norm) + 1e-6), 1)
 *                     then, in the order of torch's _single_tensor_adam (torch/optim/adam.py), every operation rounded once to fp32:
 *                       weight_decay != 0:  decoupled == 0 (Adam, L2):  g = g + weight_decay p
 *                                           decoupled != 0 (AdamW):     p = p (1 - lr weight_decay)
 *                       m = m + (1 - beta1) (g - m)                      exp_avg.lerp_(grad, 1 - beta1)
 *                       v = v beta2;  v = v + (1 - beta2) (g g)          exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
 *                       denom = sqrt(v) / sqrt(1 - beta2^step) + eps
 *                       p = p + (-(lr / (1 - beta1^step))) (m / denom)   param.addcdiv_(exp_avg, denom, value=-step_size)
 *                     The scalars 1 - beta1, 1 - beta2, 1 - lr weight_decay, lr / (1 - beta1^step), sqrt(1 - beta2^step) are formed
 *                     on the host in double, as torch forms them from Python floats, and rounded to fp32 once.
 * ---------------------------------------------------------------------------------- */
int64_t hp_head_backward_ws_floats(int B, int C, int O);
int hp_head_backward(int B, int C, int pose_dim, int n_logits, const float* d_feat, const float* d_pose_grad, const float* d_logit_grad,
                     const float* d_w, const float* d_W, int accumulate, float* d_dW, float* d_db, float* d_dfeat, float* d_ws,
                     int64_t ws_floats, void* stream);
int hp_fc_backward(int B, int O, int C, const float* d_dout, const float* d_in, int accumulate, float* d_dW, float* d_db, void* stream);
int64_t hp_grad_sq_norm_ws_floats(int64_t N);
int hp_grad_sq_norm(int64_t N, const float* d_g, float* d_sq_norm, float* d_ws, int64_t ws_floats, void* stream);
int hp_adamw_step(int64_t N, float* d_p, const float* d_g, float* d_m, float* d_v, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, int decoupled, const float* d_sq_norm, const float* d_max_norm, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HAPPYPOSE_AMD_H */
