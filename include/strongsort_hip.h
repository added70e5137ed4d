/*
 * strongsort_hip.h — C ABI of the MI355X (gfx950) StrongSORT hot path.
 *
 * The reference has no plugin / FFI interface: its only crossings into the
 * hot path are two Python calls into the third-party `ultralytics` package,
 *     /root/reference/yolo_multi_model.py:41    results = model.track(image, ..., persist=True, tracker=...)
 *     /root/reference/yolo_multi_model.py:173   results = model.predict(image, ...)
 * configured by /root/reference/yolo_multi_model.py:18-21 (conf, iou, agnostic_nms, max_det).
 * Every entry point below replaces one stage that runs inside those two calls; the Python host
 * side (strongsort_yolo_amd/yolo.py `YOLO.track/.predict`, strongsort_yolo_amd/tracker.py
 * `StrongSORT.update(dets, frame)`) binds them with ctypes — see INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes; `d_` = device memory owned by the caller; every call is
 * asynchronous on the context's HIP stream unless it says "synchronous"; return 0 or a negative
 * SS_ERR_* code, never a C++ exception; one context is not thread safe.
 *
 * The Python binding is derived from this file (strongsort_yolo_amd/cheader.py): keep to flat declarations, structs of scalars
 * and pointers, integer #defines; a `d_` pointer binds as an address, any other non-void pointer as a typed host pointer.
 */
#ifndef STRONGSORT_HIP_H
#define STRONGSORT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_OK 0
#define SS_ERR_INVALID (-1)      /* bad argument */
#define SS_ERR_CAPACITY (-2)     /* more tracks / detections / candidates than the context holds */
#define SS_ERR_HIP (-3)          /* HIP runtime error (see ss_last_error) */
#define SS_ERR_INFEASIBLE (-4)   /* assignment problem has no finite solution */

#define SS_FEAT_DIM 512
#define SS_MAX_TRACKS 256        /* track slots per stream */
#define SS_MAX_DETS 128          /* detections per stream per frame */
#define SS_OUT_COLS 8            /* x1,y1,x2,y2,track_id,class_id,conf,det_idx */

typedef struct ss_ctx ss_ctx;

/* Tracker constants (oracle/DECISIONS.md D-02..D-11).  Replaces the tracker YAML that
 * yolo_multi_model.py:41 names (`tracker="botsort.yaml"`). */
typedef struct ss_config {
    double max_dist;             /* 0.2    cosine matching threshold            */
    double max_iou_distance;     /* 0.7    IoU-stage threshold on 1-IoU          */
    double mc_lambda;            /* 0.995  appearance / motion blend            */
    double gating_threshold;     /* 9.4877 chi2inv95[4]                          */
    double gated_cost;           /* 1e5                                          */
    double std_weight_position;  /* 1/20                                         */
    double std_weight_velocity;  /* 1/160                                        */
    double ema_alpha;            /* 0.9  (a=(float)alpha, 1-a=(float)(1.0-alpha))  */
    int    max_age;              /* 30                                           */
    int    n_init;               /* 3                                            */
    int    nn_budget;            /* 100 (<= 128)                                 */
    int    n_streams;            /* independent video streams held by this context */
    int    debug;                /* !=0: keep stage intermediates for ss_get_debug */
} ss_config;

/* ---- context ------------------------------------------------------------------------------- */
int  ss_create(const ss_config* cfg, int device, ss_ctx** out);
void ss_destroy(ss_ctx* ctx);
const char* ss_last_error(const ss_ctx* ctx);            /* NULL ctx: last global error */
int  ss_set_hip_stream(ss_ctx* ctx, void* hip_stream);   /* e.g. torch.cuda.current_stream().cuda_stream */
int  ss_reset(ss_ctx* ctx, int stream);                  /* stream < 0: all streams */
int  ss_synchronize(ss_ctx* ctx);

/* Frame source side of model.track(image) (yolo_multi_model.py:272 cap.read() -> :41): copy a host frame (any pageable
 * memory, e.g. the array cv2 returned) into device memory through the context's write-combined pinned staging ring,
 * asynchronously on `hip_stream`.  The host buffer may be reused as soon as the call returns. */
int ss_upload(ss_ctx* ctx, void* hip_stream, void* d_dst, const void* h_src, size_t bytes);
/* A frame GROUP at once (the throughput form of ss_upload, for the reference's `cap.read()` loop at yolo_multi_model.py:270-278 fed
 * `batch` frames at a time): n host buffers of bytes_each bytes are staged by `threads` host threads in one write-combined area and
 * leave in ONE asynchronous copy to d_dst, where the frames lie contiguously; h_srcs may be reused on return. */
int ss_upload_batch(ss_ctx* ctx, void* hip_stream, void* d_dst, const void* const* h_srcs, int n, size_t bytes_each, int threads);

/* ... and back: device -> host through a pinned staging buffer; synchronous. */
int ss_download(ss_ctx* ctx, void* hip_stream, void* h_dst, const void* d_src, size_t bytes);

/* ---- N2  annotation overlay on device frames (the cv2 drawing of yolo_multi_model.py:58-162, :311-331) --------------
 * d_frames: `batch` BGR u8 frames [h][w][3] (row_stride bytes per row, frame b at + b*frame_batch_stride bytes), drawn in
 * place.  d_prims: primitives of all frames, 8 ints each {type, x0, y0, x1, y1, color B|G<<8|R<<16, a, b}; frame b owns
 * d_prim_off[b] .. d_prim_off[b+1] and they are painted in list order:
 *   type 0 rectangle outline, thickness a centred on the edge      type 1 filled rectangle
 *   type 2 filled circle, centre (x0,y0), radius a                 type 3 line, thickness a
 *   type 4 5x7 raster text, baseline-left (x0,y0), x1 characters at d_chars + a, scale b>>1
 *   b bit 0: member of a blended group (composited opaquely inside the group, then 0.7 : 0.3 over the frame).
 * All coverage tests are integer arithmetic (bit-exact against the NumPy rasteriser in oracle/overlay_np.py).
 * ss_overlay_set_font uploads the 95 x 5 column-bitmap font (strongsort_yolo_amd/overlay_font.py) once per context. */
int ss_overlay_set_font(ss_ctx* ctx, const uint8_t* h_font_95x5);
int ss_overlay(ss_ctx* ctx, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w,
               int row_stride, const int* d_prims, const int* d_prim_off, const uint8_t* d_chars);

/* ---- a1  letterbox / preprocess  (inside model.track/.predict, yolo_multi_model.py:41,:173) ---
 * BGR u8 [h][w][3] (row_stride bytes) -> RGB [3][out_h][out_w], /255, pad 114.
 * dst_flags: bit 0 (SS_DST_F16) writes IEEE half, else float; bit 1 (SS_DST_HWC) writes
 * channels-last [out_h][out_w][3] (what the NHWC convolutions read) instead of three planes. */
#define SS_DST_F16 1
#define SS_DST_HWC 2
#define SS_DST_U8 4   /* ss_crop_norm* with SS_DST_HWC only: uint8 output [n][256][128][3] = the rounded bilinear value per RGB channel BEFORE
                         /255 and mean / std (256 x 3 possible results: the consumer applies them — ss_op32_stem_u8); a quarter of the float bytes */
int ss_letterbox(ss_ctx* ctx, const uint8_t* d_src, int h, int w, int row_stride, void* d_dst,
                 int dst_flags, int out_h, int out_w, int new_h, int new_w, int pad_top, int pad_left,
                 int pad_value);
/* Same for `batch` equally sized images in one launch (the streams of a rank, or consecutive frames of a
 * stream): image b at d_src + b*src_batch_stride bytes, output b at d_dst + b*3*out_h*out_w elements. */
int ss_letterbox_batch(ss_ctx* ctx, const uint8_t* d_src, int batch, long long src_batch_stride, int h,
                       int w, int row_stride, void* d_dst, int dst_flags, int out_h, int out_w, int new_h,
                       int new_w, int pad_top, int pad_left, int pad_value);

/* ---- a3  NMS  (inside model.track/.predict; thresholds = yolo_multi_model.py:18-21) -----------
 * d_pred: YOLOv8 head layout [(4+nc+n_extra)][n_anchors] float (xywh, class scores, extra rows).
 * Writes up to max_det rows [x1,y1,x2,y2,conf,cls, extra...] in ORIGINAL-image pixels
 * (scale_boxes with gain/pad, clipped to w0 x h0), the kept anchor indices and the count. */
int ss_nms(ss_ctx* ctx, const float* d_pred, int n_anchors, int nc, int n_extra, float conf_thres,
           float iou_thres, int agnostic, float max_wh, int max_det, float gain, float pad_x,
           float pad_y, float w0, float h0, float* d_rows, int row_stride, int* d_keep, int* d_count);
/* `batch` images in one set of launches.  Image b: predictions at d_pred + b*pred_batch_stride floats,
 * geometry d_geom[b] = {gain, pad_x, pad_y, w0, h0} (device floats, so images of different sizes can share
 * a batch), rows at d_rows + b*rows_batch_stride floats, anchors at d_keep + b*keep_batch_stride, count
 * d_count[b].  The first call with a larger batch than any before grows the context's workspace and must
 * not be inside a HIP-graph capture.  More than 8192 candidates above conf_thres in an image leave that
 * image's count 0 and raise SS_ERR_CAPACITY at the next ss_check_errors (same for ss_nms). */
int ss_nms_batch(ss_ctx* ctx, const float* d_pred, int batch, long long pred_batch_stride, int n_anchors,
                 int nc, int n_extra, float conf_thres, float iou_thres, int agnostic, float max_wh,
                 int max_det, const float* d_geom, float* d_rows, int row_stride,
                 long long rows_batch_stride, int* d_keep, long long keep_batch_stride, int* d_count);

/* ---- oriented boxes: rotated NMS on ProbIoU (docs/OBB.md) -----------------------------------------
 * d_pred: OBB head layout [(4+nc+1)][n_anchors] float (xywh in network-input pixels, class scores, theta).  ss_nms_batch's
 * arguments without max_wh: classes are separated by equality, not by an offset (R-03).  A candidate is removed when ANY
 * higher-scored candidate has ProbIoU >= iou_thres with it (R-02, Ultralytics' nms_rotated; not a greedy scan).  Writes up to
 * max_det rows [x1,y1,x2,y2,conf,cls, cx,cy,w,h,theta] (row_stride >= 11) in ORIGINAL-image pixels: the rotated box is
 * scaled, not clipped, and regularised (w >= h, theta in [0, pi)); columns 0..3 are its axis-aligned envelope clipped to the
 * image, so columns 0..5 read as a plain detection row.  Candidate filter, `classes` mask, d_keep, d_count, the workspace
 * growth outside a capture and the 8192-candidate capacity are ss_nms_batch's.  Asynchronous and capturable. */
int ss_nms_obb_batch(ss_ctx* ctx, const float* d_pred, int batch, long long pred_batch_stride, int n_anchors,
                     int nc, float conf_thres, float iou_thres, int agnostic, int max_det, const float* d_geom,
                     float* d_rows, int row_stride, long long rows_batch_stride, int* d_keep,
                     long long keep_batch_stride, int* d_count);
/* Known-answer entry, synchronous: ProbIoU of every pair of the HOST lists h_a [n][5] and h_b [m][5] (cx, cy, w, h, theta;
 * n, m <= 4096) by the device function the rotated NMS uses, into the host matrix h_out [n][m].  A box with a non-finite
 * field, w <= 0, h <= 0 or |theta| > 2^20 has ProbIoU 0 with everything (R-01). */
int ss_probiou(ss_ctx* ctx, const float* h_a, int n, const float* h_b, int m, double* h_out);

/* The `classes` override of the reference (yolo_multi_model.py:22, commented out there): keep only anchors whose best
 * class is in classes[0..n) (ids 0..127); n = 0 keeps every class (default).  Host state of the context, read by the
 * following ss_nms / ss_nms_batch calls (and baked into a HIP graph that captures them). */
int ss_nms_set_classes(ss_ctx* ctx, const int* classes, int n);

/* ---- a4  ReID crop-extract  (StrongSORT._get_features, inside model.track) ---------------------
 * For each detection row (x1,y1,x2,y2,... ; det_stride floats) crop + bilinear to 256x128,
 * /255, ImageNet mean/std, RGB [n][3][256][128] (out_flags as ss_letterbox's dst_flags: SS_DST_F16,
 * SS_DST_HWC for [n][256][128][3]).  Rows >= *d_count are left untouched when d_count != NULL. */
int ss_crop_norm(ss_ctx* ctx, const uint8_t* d_frame, int h, int w, int row_stride,
                 const float* d_dets, int det_stride, int n, const int* d_count, void* d_out,
                 int out_flags);
/* `batch` frames in one launch: frame b at d_frames + b*frame_batch_stride bytes, its detections at
 * d_dets + b*dets_batch_stride floats, its count d_counts[b] (NULL: n each), output [batch][n][3][256][128]. */
int ss_crop_norm_batch(ss_ctx* ctx, const uint8_t* d_frames, int batch, long long frame_batch_stride,
                       int h, int w, int row_stride, const float* d_dets, int det_stride,
                       long long dets_batch_stride, int n, const int* d_counts, void* d_out, int out_flags);
/* Packed form of ss_crop_norm_batch (channels-last output only): d_off [batch + 1] receives the exclusive prefix of
 * min(count, n) (d_off[batch] = number of crops) and crop d of image i lands at slot d_off[i] + d, so the valid crops of
 * a frame group are contiguous; ss_op_set_valid_images(stream, d_off + batch, batch * n) then lets the ReID network skip the rest.
 * ss_unpack_feats: d_feats[i][d][0..512) (float, image stride in floats) = d_emb[d_off[i] + d] for d < min(count, n). */
int ss_crop_norm_packed(ss_ctx* ctx, const uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int stride,
                        const float* d_dets, int det_stride, long long dets_batch_stride, int n, const int* d_counts,
                        int* d_off, void* d_out, int out_flags);
int ss_unpack_feats(ss_ctx* ctx, const void* d_emb, int emb_half, const int* d_off, const int* d_counts, int batch, int n,
                    float* d_feats, long long feats_image_stride);

/* One frame's results gathered into ONE buffer on the context's stream (the per-frame call of yolo_multi_model.py:41 / :278 reads boxes and
 * track rows on the host after every frame): d_dst[0] = n = min(*d_n_dets, det_cap) and d_dst[1] = m = min(*d_n_out, out_cap) as int32 bit
 * patterns, n rows of det_ld floats from d_dst + 2, m rows of out_ld floats from d_dst + 2 + det_cap * det_ld.  d_dst: 2 + det_cap * det_ld +
 * out_cap * out_ld floats of device memory or of pinned (device-accessible) host memory - then the host reads it after synchronising the
 * stream, with no copy in between.  d_n_out / d_out may both be NULL (detection only: m = 0). */
int ss_pack_results(ss_ctx* ctx, const int* d_n_dets, const float* d_dets, int det_ld, int det_cap, const int* d_n_out, const float* d_out,
                    int out_ld, int out_cap, float* d_dst);

/* ---- instance masks of a segmentation head (yolo.py assemble_masks / mask_polygon on the device; YOLO(device_masks=True)) --------
 * ss_mask_assemble: frame f's prototypes at d_proto + f*proto_frame_stride elements ([nm][mh][mw], IEEE half when proto_f16, else
 * float), its detection rows at d_dets + f*dets_frame_stride floats ([max_rows][det_ld]: x1,y1,x2,y2 in original pixels, the nm
 * coefficients from column coef_off), its geometry d_geom + f*geom_frame_stride = {gain, pad_x, pad_y} (0: shared by all frames).
 * For the rows below min(d_counts[f], max_rows): box = x * gain + pad, cropped linear combination on the prototype grid, bilinear
 * (align_corners = false) to ih x iw = 4 mh x 4 mw, > 0, in the float32 order tests/test_masks_device_cpu.py restates.  Writes whole
 * bit planes uint32 [max_rows][ih][ceil(iw/32)] at d_bits + f*bits_frame_stride words (bit x%32 of word x/32 = pixel (y, x)); rows
 * at or beyond the count are not written.  Constraints: 1 <= nm <= 64, mw <= 256.
 * ss_mask_outline: for the same rows of packed planes (layout as above), the polygon yolo.mask_polygon returns: d_pts + f*pts_frame_stride
 * int32 [max_rows][cap][2] (x, y) and d_npts[f*npts_frame_stride + r] = its length, or -length (no points written) when longer than
 * cap.  d_bits_copy (NULL: none) receives a copy of each processed plane (e.g. pinned host memory, layout as d_bits with
 * copy_frame_stride).  d_scratch: scratch_bytes of device memory, at least one label plane of 4 * ih * iw bytes; every whole plane in
 * it serves one workgroup (at most 1024).  ih * ceil(iw/32) <= 12800.
 * Both check every argument before the context: a bad call returns SS_ERR_INVALID without touching the device, even with ctx NULL. */
int ss_mask_assemble(ss_ctx* ctx, void* hip_stream, const void* d_proto, int proto_f16, long long proto_frame_stride, int nm, int mh, int mw,
                     const float* d_dets, long long dets_frame_stride, int det_ld, int coef_off, const int* d_counts, int n_frames,
                     int max_rows, const float* d_geom, long long geom_frame_stride, int ih, int iw, uint32_t* d_bits,
                     long long bits_frame_stride);
int ss_mask_outline(ss_ctx* ctx, void* hip_stream, const uint32_t* d_bits, long long bits_frame_stride, const int* d_counts, int n_frames,
                    int max_rows, int ih, int iw, int cap, int* d_pts, long long pts_frame_stride, int* d_npts, long long npts_frame_stride,
                    uint32_t* d_bits_copy, long long copy_frame_stride, void* d_scratch, long long scratch_bytes);

/* Largest n_frames ss_track_update_group / ss_cmc_estimate accept (compile-time SS_FMAX). */
int ss_max_group_frames(void);
/* hip_event (a hipEvent_t of the caller, NULL: none) is recorded on the tracker's stream right after the association launch
 * of every following ss_track_update_group call: a pipeline can hold its other stream back for those ~40 us — the
 * association kernel needs whole CUs (8 waves x 127 VGPRs + 64 KiB LDS per workgroup) and is starved by co-running network
 * kernels otherwise — and let it run beside the per-frame chain that follows. */
int ss_track_set_assoc_event(ss_ctx* ctx, void* hip_event);
/* ---- a6..a10  tracker update  (tracker.update inside model.track, yolo_multi_model.py:41) -----
 * A GROUP of n_frames (1..ss_max_group_frames() = 32) consecutive frames for EVERY stream of the context in one batch of launches; the
 * frames are associated strictly in order (frame f sees the tracks, galleries and ids left by frame f-1), so the
 * rows are identical to n_frames single-frame calls — what the group buys is that the galleries are read from HBM
 * once per group instead of once per frame (the association kernel handles the detections of all frames at once).
 *   d_dets   [n_frames][n_streams][SS_MAX_DETS][6]   x1,y1,x2,y2,conf,cls (original pixels, float)
 *   d_ndets  [n_frames][n_streams]                   detections per frame and stream (device ints)
 *   d_feats  [n_frames][n_streams][SS_MAX_DETS][512] raw ReID embeddings (normalised on device)
 *   d_img_hw [n_streams][2]                          frame height, width (device ints; output clipping)
 * Results stay on the device: d_out [n_frames][n_streams][SS_MAX_TRACKS][8], d_nout [n_frames][n_streams].
 * Device-side capacity errors: detections of a frame that would need more than SS_MAX_TRACKS slots start no track (the
 * frame is tracked as if they had not been there); the stream's tables stay consistent, SS_ERR_CAPACITY is reported by the
 * next ss_check_errors and stays set until ss_reset. */
int ss_track_update_group(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats,
                          const int* d_img_hw, float* d_out, int* d_nout);
/* One frame: ss_track_update_group with n_frames = 1. */
int ss_track_update(ss_ctx* ctx, const float* d_dets, const int* d_ndets, const float* d_feats,
                    const int* d_img_hw, float* d_out, int* d_nout);

/* ---- BYTE tracker family (docs/BYTETRACK.md): ByteTrack (xyah Kalman) and BoT-SORT (xywh Kalman, optional GMC and ReID) -----
 * Opt-in association on IoU and detection scores; BoT-SORT can add an appearance term (ss_byte_set_reid).  The state is hung off an existing context (its streams,
 * its HIP stream, its error words); ss_byte_create on a context that already has one replaces it. */
typedef struct ss_byte_config {
    double track_high_thresh;    /* 0.25  first-association rows: score >= this                   */
    double track_low_thresh;     /* 0.1   second-association rows: low < score < high              */
    double new_track_thresh;     /* 0.25  births: score >= this                                     */
    double match_thresh;         /* 0.8   first association: fused 1-IoU <= this                    */
    double std_weight_position;  /* 1/20                                                             */
    double std_weight_velocity;  /* 1/160                                                            */
    int    track_buffer;         /* 30    max_time_lost = int(frame_rate / 30 * track_buffer)         */
    int    frame_rate;           /* 30                                                               */
    int    fuse_score;           /* 1     cost = 1 - (1 - cost) * score in the fused stages           */
    int    kalman_xywh;          /* 0 xyah (ByteTrack), 1 xywh (BoT-SORT)                            */
    int    max_tracks;           /* <= SS_MAX_TRACKS per stream (tracked + lost + unconfirmed)        */
    int    max_dets;             /* <= SS_MAX_DETS per frame                                         */
} ss_byte_config;
int ss_byte_create(ss_ctx* ctx, const ss_byte_config* cfg);
int ss_byte_destroy(ss_ctx* ctx);
/* A group of n_frames (1..32) frames of every stream in ONE launch, associated strictly in order; layouts as
 * ss_track_update_group without features: d_dets [n_frames][n_streams][SS_MAX_DETS][6], d_ndets [n_frames][n_streams] ->
 * d_out [n_frames][n_streams][SS_MAX_TRACKS][8] (x1,y1,x2,y2,track_id,class_id,conf,det_idx; det_idx >= 0 always),
 * d_nout [n_frames][n_streams].  Asynchronous on the context's stream, capturable.  A frame with more than max_dets rows is
 * tracked on its first max_dets; births beyond max_tracks are dropped; either raises SS_ERR_CAPACITY at ss_check_errors
 * (set until ss_byte_reset). */
int ss_byte_update_group(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_byte_update(ss_ctx* ctx, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_byte_reset(ss_ctx* ctx, int stream);                /* stream < 0: all streams; ids restart at 1, frame_id at 1; the
                                                              stream's previous ss_cmc_estimate / ss_gmc_sparse_estimate frame is forgotten (no warp next)
                                                              and its ReID track features and stored poses are cleared */
/* BoT-SORT GMC (docs/BYTETRACK.md §1b): the following ss_byte_update(_group) calls move every track's Kalman mean and covariance
 * by d_warps[f][s][8] (ss_cmc_estimate's layout; [6] < 0: no warp) after predicting frame f.  The caller keeps at least
 * n_frames rows alive; the pointer is read at launch (capturable).  NULL switches it off (the default).  SS_ERR_INVALID without
 * BYTE state or on an xyah (ByteTrack) state. */
int ss_byte_set_gmc(ss_ctx* ctx, const double* d_warps);
/* BoT-SORT's ReID branch (docs/BYTETRACK.md §1c): on != 0 adds the appearance term to the first and third associations, with
 * proximity_thresh (0.5, on 1 - IoU), appearance_thresh (0.25, on the halved cosine distance) and the feature EMA weight alpha
 * (0.9: (float)alpha, (float)(1 - alpha)).  Switching (on or off) resets every stream.  The first switch-on allocates the track
 * features (512 KiB per stream) and the group's unit features (8 MiB per stream).  SS_ERR_INVALID without BYTE state or on an
 * xyah (ByteTrack) state.  While ReID is on, ss_byte_update(_group) are refused: use ss_byte_update_group_feats. */
int ss_byte_set_reid(ss_ctx* ctx, int on, double proximity_thresh, double appearance_thresh, double alpha);
/* ss_byte_update_group with the group's raw detection features d_feats [n_frames][n_streams][SS_MAX_DETS][512] f32 (ReID on;
 * ignored and may be NULL when it is off).  Asynchronous, capturable. */
int ss_byte_update_group_feats(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats,
                               float* d_out, int* d_nout);
/* Synchronous: the unit track features [n][512] of one stream in ss_byte_get_tracks' list order (after ss_byte_set_reid). */
int ss_byte_get_features(ss_ctx* ctx, int stream, int cap, float* smooth);
/* The keypoint (OKS) term of BoT-SORT (docs/BYTETRACK.md §1e, this project's own definition): on != 0 adds an OKS entry to the first
 * and third associations for the pairs with 1 - IoU <= proximity_thresh (0.5), kept when (1 - OKS) / 2 <= pose_thresh (0.25); a
 * keypoint counts when its visibility >= (float)vis_thresh (0.5), a pair when at least min_common (3) count on both sides; sigmas:
 * n_kpt (1..32) host doubles (COCO's 17).  Switching (on or off) resets every stream.  The first switch-on allocates the pose tables.
 * SS_ERR_INVALID without BYTE state, on an xyah (ByteTrack) state, while ReID is on, or with n_kpt outside 1..32.  While it is on,
 * ss_byte_update(_group) and ss_byte_update_group_feats are refused (use ss_byte_update_group_kpts), and so is ss_byte_set_reid(on). */
int ss_byte_set_pose(ss_ctx* ctx, int on, int n_kpt, const double* sigmas, double proximity_thresh, double pose_thresh,
                     double vis_thresh, int min_common);
/* ss_byte_update_group with the group's keypoints: row r of image i = f * n_streams + s at d_kpts + (i * SS_MAX_DETS + r) *
 * kpt_row_stride + kpt_col_offset floats, n_kpt triplets (x, y, visibility) f32 (NMS rows carry them at column 6).  d_geom
 * [n_frames * n_streams][5] = ss_nms_batch's geometry rows {gain, pad_x, pad_y, ..}: the keypoints are network-input pixels and are
 * brought to original pixels, (x - pad) / gain in float32; NULL: they are original pixels already.  Asynchronous, capturable. */
int ss_byte_update_group_kpts(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, const float* d_kpts,
                              long long kpt_row_stride, int kpt_col_offset, const float* d_geom, float* d_out, int* d_nout);
/* Synchronous: the stored poses of one stream in ss_byte_get_tracks' list order: offsets [n][n_kpt][2] f64 (from the box centre, in
 * box widths / heights) and one visibility word per track (bit k = keypoint k); either may be NULL. */
int ss_byte_get_keypoints(ss_ctx* ctx, int stream, int cap, double* offsets, unsigned* visible);
/* Oriented boxes (docs/OBB.md §4): on != 0 swaps the cost of the three associations and of the duplicate test for 1 - ProbIoU of the
 * rotated boxes; every track remembers the angle of its last row (R-06), the Kalman filter is unchanged.  Resets every stream.
 * Allocates the per-slot angles and the boxes' ProbIoU terms on the first switch-on.  SS_ERR_INVALID without BYTE state or while ReID,
 * the keypoint term or GMC is on (and those refuse while this is on).  While it is on, ss_byte_update(_group) and
 * ss_byte_update_group_feats are refused: use ss_byte_update_group_obb. */
int ss_byte_set_obb(ss_ctx* ctx, int on);
/* ss_byte_update_group on ss_nms_obb_batch's rows: d_dets [n_frames][n_streams][SS_MAX_DETS][11] = x1, y1, x2, y2, conf, cls, cx, cy,
 * w, h, theta (columns 0..3 are not read).  d_out as ss_byte_update_group's, columns 0..3 the axis-aligned envelope (not clipped) of
 * the track's rotated box; d_out_rbox [n_frames][n_streams][SS_MAX_TRACKS][5] = cx, cy, w, h, theta of the same rows.  One launch:
 * capturable. */
int ss_byte_update_group_obb(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, float* d_out_rbox,
                             int* d_nout);
/* Synchronous: the angles [n] of one stream's tracks in ss_byte_get_tracks' list order (after ss_byte_set_obb). */
int ss_byte_get_angles(ss_ctx* ctx, int stream, int cap, float* angles);
/* Synchronous inspection call, a permanent part of this ABI like ss_get_debug (the tests compare k_byte_kpts' output through it bit
 * for bit): the detection keypoints of image (frame, stream) as the last ss_byte_update_group_kpts call prepared them:
 * xy [SS_MAX_DETS][n_kpt][2] f32 in original pixels, visibility words [SS_MAX_DETS]; rows past the image's count are not written. */
int ss_byte_get_det_keypoints(ss_ctx* ctx, int frame, int stream, float* xy, unsigned* visible);
/* BoT-SORT's `model: auto` ReID features (docs/BYTETRACK.md §1d): the raw features of kept detections read from the detector's
 * own head inputs.  maps[3]: the levels P3, P4, P5 of n_img images (f16 if half, else f32), channel stride 1, element (i, c, y, x)
 * at data + i*img_stride + y*row_stride + x*pix_stride + c (strides in elements; a channel slice of a wider map is fine).
 * d_keep [n_img][keep_stride] (>= SS_MAX_DETS): NMS anchor indices (level by level, row-major inside a level), d_counts [n_img].
 * d_out [n_img][SS_MAX_DETS][512] f32: for r < min(count, SS_MAX_DETS), columns j < s hold the mean of channels [j*g, (j+1)*g)
 * of every level (g = channels / s; f32 sum in channel order, then / g) and columns s..511 zeros; rows past the count are not
 * written.  1 <= s <= 512 and channels % s == 0 on every level.  Asynchronous on the context's stream, capturable; every
 * argument is checked first (SS_ERR_INVALID without touching the device). */
typedef struct ss_native_map {
    const void* data;
    long long img_stride, row_stride, pix_stride;
    int channels, height, width;
} ss_native_map;
int ss_native_feats(ss_ctx* ctx, int n_img, int half, const ss_native_map* maps, int s, const int* d_keep, long long keep_stride,
                    const int* d_counts, float* d_out);
/* Synchronous: the table of one stream in list order (tracked list, then lost list); any array may be NULL.
 * state 1 tracked, 2 lost; mean [n][8] (xyah or xywh state). */
int ss_byte_get_tracks(ss_ctx* ctx, int stream, int cap, int* n_tracked, int* n_lost, int* next_id, int* frame_id,
                       int* track_id, int* state, int* activated, double* mean);

/* ---- OC-SORT (docs/OCSORT.md): the motion-only tracker with observation-centric re-update, momentum and recovery ----------------
 * A 7-state SORT Kalman filter per track and IoU association with a direction-consistency term; no weights, no frames.  The state
 * is hung off an existing context like the BYTE state (the two may coexist); ss_ocsort_create on a context that already has one
 * replaces it.  SS_ERR_INVALID unless 1 <= max_tracks <= SS_MAX_TRACKS, 1 <= max_dets <= SS_MAX_DETS, 1 <= delta_t <= 8,
 * max_age >= 1, min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0 and use_byte is 0 or 1. */
typedef struct ss_ocsort_config {
    double det_thresh;           /* 0.25  first association and births: score > this                          */
    double low_thresh;           /* 0.1   BYTE stage rows: low < score < det_thresh                            */
    double iou_threshold;        /* 0.3   a pair is kept when its IoU >= this                                  */
    double inertia;              /* 0.2   weight of the direction-consistency term                             */
    int    max_age;              /* 30    a track is removed when time_since_update > this                     */
    int    min_hits;             /* 3     rows need hit_streak >= this (or frame_count <= this)                */
    int    delta_t;              /* 3     observations this many ages back give the directions (1..8)          */
    int    use_byte;             /* 0     1: the second association on the low-score rows                      */
    int    max_tracks;           /* <= SS_MAX_TRACKS per stream                                                */
    int    max_dets;             /* <= SS_MAX_DETS per frame                                                   */
} ss_ocsort_config;
int ss_ocsort_create(ss_ctx* ctx, const ss_ocsort_config* cfg);
int ss_ocsort_destroy(ss_ctx* ctx);
/* A group of n_frames (1..32) frames of every stream in ONE launch, associated strictly in order; the layouts of
 * ss_byte_update_group: d_dets [n_frames][n_streams][SS_MAX_DETS][6], d_ndets [n_frames][n_streams] ->
 * d_out [n_frames][n_streams][SS_MAX_TRACKS][8] (x1,y1,x2,y2,track_id,class_id,conf,det_idx; the box is the track's last
 * observation, newest track first; det_idx >= 0 always), d_nout [n_frames][n_streams].  Every argument is checked first
 * (SS_ERR_INVALID without touching the device).  Asynchronous on the context's stream, capturable.  A frame with more than
 * max_dets rows is tracked on its first max_dets; births beyond max_tracks are dropped; either raises SS_ERR_CAPACITY at
 * ss_check_errors (set until ss_ocsort_reset). */
int ss_ocsort_update_group(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_ocsort_update(ss_ctx* ctx, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_ocsort_reset(ss_ctx* ctx, int stream);              /* stream < 0: all streams; ids restart at 1, frame_count at 0 */
/* Synchronous: the table of one stream in list order (oldest track first); any array may be NULL.  x [n][7] (x, y, s, r, vx, vy,
 * vs), P [n][49], frozen: 1 while the filter holds a copy frozen at the first miss after an observation, last_obs [n][4] xyxy
 * (-1 four times while the track has none), velocity [n][2] unit direction (x, y; zeros while none). */
int ss_ocsort_get_tracks(ss_ctx* ctx, int stream, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                         int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                         double* velocity);

/* ---- Hybrid-SORT (docs/HYBRIDSORT.md): OC-SORT's machinery with the confidence as a Kalman state and a cost term (TCM), the
 * height-modulated IoU and the direction term over the four box corners and delta_t time offsets ------------------------------
 * No weights, no frames.  The state is hung off an existing context like the OC-SORT state (they may coexist);
 * ss_hybridsort_create on a context that already has one replaces it.  SS_ERR_INVALID unless 1 <= max_tracks <= SS_MAX_TRACKS,
 * 1 <= max_dets <= SS_MAX_DETS, 1 <= delta_t <= 8, max_age >= 1, min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0, both TCM
 * weights >= 0, low_thresh <= det_thresh, and use_byte and hmiou are 0 or 1. */
typedef struct ss_hybridsort_config {
    double det_thresh;           /* 0.25  first association and births: score > this                          */
    double low_thresh;           /* 0.1   BYTE stage rows: low < score < det_thresh                            */
    double iou_threshold;        /* 0.3   a pair is kept when its (height-modulated) IoU >= this               */
    double inertia;              /* 0.05  weight of each corner's direction-consistency term                   */
    double tcm_first_weight;     /* 1.0   weight of |score - Kalman confidence| in the first association       */
    double tcm_byte_weight;      /* 1.0   weight of |score - linear confidence| in the BYTE stage              */
    int    max_age;              /* 30    removed when time_since_update > max_age                             */
    int    min_hits;             /* 3     shown from this hit streak on (and during the first min_hits frames) */
    int    delta_t;              /* 3     time offsets of the direction term, 1..8                             */
    int    use_byte;             /* 1     1: the second association on the low-score rows                      */
    int    hmiou;                /* 1     1: height-modulated IoU, 0: IoU                                      */
    int    max_tracks;           /* <= SS_MAX_TRACKS per stream                                                */
    int    max_dets;             /* <= SS_MAX_DETS per frame                                                   */
} ss_hybridsort_config;
int ss_hybridsort_create(ss_ctx* ctx, const ss_hybridsort_config* cfg);
int ss_hybridsort_destroy(ss_ctx* ctx);
/* A group of n_frames (1..32) frames of every stream in ONE launch: the layouts, checks and capacity errors of
 * ss_ocsort_update_group (set until ss_hybridsort_reset).  Asynchronous on the context's stream, capturable. */
int ss_hybridsort_update_group(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_hybridsort_update(ss_ctx* ctx, const float* d_dets, const int* d_ndets, float* d_out, int* d_nout);
int ss_hybridsort_reset(ss_ctx* ctx, int stream);          /* stream < 0: all streams; ids restart at 1, frame_count at 0 */
/* Synchronous: the table of one stream in list order (oldest track first); any array may be NULL.  x [n][9] (x, y, s, c, r, vx,
 * vy, vs, vc), P [n][81] (entries outside the components' blocks are +0.0), frozen as ss_ocsort_get_tracks, last_obs [n][4] xyxy
 * (-1 four times while the track has none), velocity [n][8] the corners' direction sums (lt, rt, lb, rb; x, y; zeros while none),
 * conf [n] the score of the last match (the birth row's before any), conf_prev [n] of the match before it (-1 while none). */
int ss_hybridsort_get_tracks(ss_ctx* ctx, int stream, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                             int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                             double* velocity, float* conf, float* conf_prev);

/* ---- Deep OC-SORT (docs/DEEPOCSORT.md): OC-SORT with camera-motion compensation, dynamic appearance and adaptive weighting -------
 * OC-SORT's frame procedure without the BYTE stage; the first association adds w_association_emb x (adaptive weight) x the
 * similarity of the row's unit feature and the track's feature, and every track keeps a feature whose EMA weight follows the
 * detection score.  The state is hung off an existing context like the BYTE and OC-SORT states (they may coexist);
 * ss_deepoc_create on a context that already has one replaces it.  SS_ERR_INVALID unless 1 <= max_tracks <= SS_MAX_TRACKS,
 * 1 <= max_dets <= SS_MAX_DETS, 1 <= delta_t <= 8, max_age >= 1, min_hits >= 0, 0 < iou_threshold <= 1, inertia >= 0,
 * det_thresh < 1, w_association_emb >= 0, 0 <= alpha_fixed_emb <= 1, 0 <= aw_param < 1 and the three flags are 0 or 1.  It
 * allocates the track features (512 KiB per stream), the group's unit features (8 MiB per stream) and the similarities. */
typedef struct ss_deepoc_config {
    double det_thresh;           /* 0.25  first association and births: score > this; the zero of the score's trust */
    double iou_threshold;        /* 0.3   a pair is kept when its IoU >= this                                  */
    double inertia;              /* 0.2   weight of the direction-consistency term                             */
    double w_association_emb;    /* 0.75  weight of the appearance cost                                        */
    double alpha_fixed_emb;      /* 0.95  the feature EMA's weight at trust 1 (and always, without dynamic_appearance) */
    double aw_param;             /* 0.5   adaptive weighting: second / first similarity above this lowers the weight */
    int    max_age;              /* 30    a track is removed when time_since_update > this                     */
    int    min_hits;             /* 3     rows need hit_streak >= this (or frame_count <= this)                */
    int    delta_t;              /* 3     observations this many ages back give the directions (1..8)          */
    int    appearance;           /* 1     0: no appearance cost and no features (d_feats is not read)          */
    int    dynamic_appearance;   /* 1     the EMA weight follows the detection score                           */
    int    adaptive_weighting;   /* 1     per-row and per-track factors on w_association_emb                   */
    int    max_tracks;           /* <= SS_MAX_TRACKS per stream                                                */
    int    max_dets;             /* <= SS_MAX_DETS per frame                                                   */
} ss_deepoc_config;
int ss_deepoc_create(ss_ctx* ctx, const ss_deepoc_config* cfg);
int ss_deepoc_destroy(ss_ctx* ctx);
/* A group of n_frames (1..32) frames of every stream, associated strictly in order; the layouts of ss_byte_update_group_feats:
 * d_dets [n_frames][n_streams][SS_MAX_DETS][6], d_ndets [n_frames][n_streams], d_feats [n_frames][n_streams][SS_MAX_DETS][512] f32
 * raw features (only the rows scoring above det_thresh are read; NULL allowed when appearance is 0) -> d_out
 * [n_frames][n_streams][SS_MAX_TRACKS][8] and d_nout as ss_ocsort_update_group.  Every argument is checked first (SS_ERR_INVALID
 * without touching the device).  Asynchronous on the context's stream, capturable.  Capacity errors as ss_ocsort_update_group
 * (set until ss_deepoc_reset). */
int ss_deepoc_update_group(ss_ctx* ctx, int n_frames, const float* d_dets, const int* d_ndets, const float* d_feats, float* d_out,
                           int* d_nout);
int ss_deepoc_update(ss_ctx* ctx, const float* d_dets, const int* d_ndets, const float* d_feats, float* d_out, int* d_nout);
/* Camera-motion compensation (docs/DEEPOCSORT.md step 1b): the following update calls move every track's filter, frozen filter,
 * last observation and recent observations by d_warps[f][s][8] (ss_cmc_estimate's layout; [6] < 0: no warp) before predicting
 * frame f.  The caller keeps at least n_frames rows alive; the pointer is read at launch (capturable).  NULL switches it off
 * (the default).  SS_ERR_INVALID without Deep OC-SORT state. */
int ss_deepoc_set_gmc(ss_ctx* ctx, const double* d_warps);
int ss_deepoc_reset(ss_ctx* ctx, int stream);              /* stream < 0: all streams; ids restart at 1, frame_count at 0; the stream's
                                                              previous ss_cmc_estimate / ss_gmc_sparse_estimate frame is forgotten (no warp
                                                              next) and its track features are cleared */
/* Synchronous: the table of one stream in list order, the fields of ss_ocsort_get_tracks. */
int ss_deepoc_get_tracks(ss_ctx* ctx, int stream, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id, int* age,
                         int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P, float* last_obs,
                         double* velocity);
/* Synchronous: the tracks' unit features [n][512] of one stream in ss_deepoc_get_tracks' list order (zeros while appearance is 0). */
int ss_deepoc_get_features(ss_ctx* ctx, int stream, int cap, float* emb);

/* ---- N4  camera-motion compensation (upstream StrongSORT: tracker.camera_update(prev, cur) before tracker.predict();
 * not in the reference snapshot; optional) ----------------------------------------------------------
 * ss_cmc_estimate: for the n_frames x n_streams BGR u8 frames at d_frames ([F][S] order, frame_stride bytes apart) build
 * the 0.1x grey images and align each with its predecessor (the stream's last frame of the previous call for f = 0) by
 * ECC, euclidean warp, <= 100 iterations: d_warps[f][s][8] = 2x3 matrix previous -> current in full-frame pixels,
 * [6] = iterations (>= 1) or -1 (no usable alignment / no predecessor: identity), [7] = 0.  Asynchronous on hip_stream;
 * stateless apart from the remembered last frames, so it can run beside the detector.  d_n_valid (device int, may be NULL =
 * n_frames): only the first *d_n_valid frames of the buffer are real (a partial last group behind a captured graph): the
 * others get -1 warps and the last REAL frame is what the next call aligns its first frame with.  20 <= h, w; row_stride >= 3 * w;
 * n_frames <= ss_max_group_frames(); the first call for a frame size allocates (not inside a graph capture) and forgets every
 * stream's predecessor.
 * ss_cmc_get_small: synchronous inspection call, a permanent part of this ABI like ss_gmc_sparse_get (the tests compare the small
 * images through it byte for byte).  The hs x ws grey image (hs = (int)(h * 0.1), ws = (int)(w * 0.1), rows ws bytes apart) of
 * `stream`: frame 0 = the remembered predecessor (after a call: the call's last real frame), frame 1..n_frames = the frames of the
 * last ss_cmc_estimate.  out may be NULL (only *hs, *ws are written; either may be NULL); otherwise cap >= hs * ws bytes.
 * SS_ERR_INVALID before the first ss_cmc_estimate, for a frame / stream out of range and for a cap too small.
 * ss_track_set_cmc: the following tracker calls move every track's box by warp [f][s] before predicting frame f
 * (NULL switches compensation off, the default). */
int ss_cmc_estimate(ss_ctx* ctx, void* hip_stream, const uint8_t* d_frames, int n_frames, long long frame_stride, int h, int w,
                    int row_stride, const int* d_n_valid, double* d_warps);
int ss_cmc_get_small(ss_ctx* ctx, int frame, int stream, uint8_t* out, int cap, int* hs, int* ws);
int ss_track_set_cmc(ss_ctx* ctx, const double* d_warps);

/* ---- BoT-SORT GMC by sparse optical flow (docs/BYTETRACK.md §1f, decisions S-01..; Ultralytics' gmc_method: sparseOptFlow,
 * restated) ----------------------------------------------------------------------------------------------------------
 * ss_gmc_sparse_estimate: ss_cmc_estimate's contract and output layout with another estimator.  For the n_frames x n_streams BGR
 * u8 frames at d_frames ([F][S] order, frame_stride bytes apart): the half-size grey image and three pyrDown levels, up to 1000
 * Shi-Tomasi corners per image (computed once, they serve the pair with the next frame), pyramidal Lucas-Kanade (21 x 21 window,
 * levels 3..0, <= 30 iterations) from each frame's predecessor (the stream's last real frame of the previous call for f = 0), and a
 * similarity fit (1024 two-point hypotheses, 3 px inlier bound, closed-form refit).  d_warps[f][s][8] = 2x3 matrix previous ->
 * current in full-frame pixels, [6] = inliers (>= 2) or -1 with the identity stored (no predecessor: first frame or after
 * ss_reset / ss_byte_reset; fewer than 5 tracked corners; an image of the pair without a corner; a frame past *d_n_valid),
 * [7] = tracked corners.  Asynchronous on hip_stream and capturable once the first call for a frame size has been made outside a
 * capture (it allocates).  d_n_valid: as ss_cmc_estimate.  64 <= h, w <= 16384 (level 3 of the half image is at least 4 x 4),
 * row_stride >= 3 * w; every argument is checked before the context and the device: SS_ERR_INVALID, even with ctx NULL.
 * ss_gmc_sparse_get: synchronous inspection call, a permanent part of this ABI like ss_get_debug (the tests compare every stage
 * through it bit for bit).  For the pair (frame, stream) of the last estimate: the current image's half-size grey image and its
 * three lower levels (sizes: w/2 x h/2, then (n + 1) / 2 per level); the previous image's corners [n][2] (x, y) in selection
 * order, their count and the number of candidates before the cut to 1000; the corners' tracked positions [1000][2] (half-size
 * pixels), status bytes [1000] and inlier mask [1000].  Any pointer may be NULL. */
int ss_gmc_sparse_estimate(ss_ctx* ctx, void* hip_stream, const uint8_t* d_frames, int n_frames, long long frame_stride, int h, int w,
                           int row_stride, const int* d_n_valid, double* d_warps);
int ss_gmc_sparse_get(ss_ctx* ctx, int frame, int stream, uint8_t* half, uint8_t* level1, uint8_t* level2, uint8_t* level3,
                      int* corners_xy, int* n_corners, int* n_candidates, double* points, uint8_t* status, uint8_t* inliers);

/* Synchronous convenience for one stream with host buffers (used by StrongSORT.update). */
int ss_track_update_host(ss_ctx* ctx, int stream, const float* h_dets, int n, const float* h_feats,
                         int img_h, int img_w, float* h_out, int cap_rows, int* n_out);

/* Tuning switches of a context (host state, read at the next tracker call):
 *   "cos_grid"         persistent workgroups of the association kernel, a multiple of 8 (default 512 = two per CU)
 *   "assoc_comp_rows"  a gallery's last 16-row tile with at most this many rows (0..12, default 12) is cut into 4-row groups
 *                      and four groups of any tracks form one composite tile of the association kernel (0: off)
 *   "assoc_stage"      how the association kernel brings a work record's detection operand (2 x 32 KiB) into the LDS:
 *                      0 through registers behind one barrier; 1 / 2 / 4 by LDS-DMA in that many pieces, each awaited
 *                      right before the first k-segment that reads it; 5 = 4 with only the first piece requested before
 *                      the first barrier (default).  Same bits in every form.
 *   "track_graph"      1 (default): the per-frame chain of a group of >= 2 frames (k_frame / k_post / k_newrow, 3 F - 1 dependent
 *                      launches) is replayed as one captured HIP graph per (frames, caller buffers, options) combination — one
 *                      hipGraphLaunch of host time instead of up to 95 launches; 0: plain launches
 *   "assoc_xcd_map"    0 (default): a gallery range lives on one XCD (every XCD stages all detection operands);
 *                      1: a detection column-tile pair lives on one XCD (every XCD streams the whole gallery)
 *   "frame_caps"       0 (default) or a multiple of 16 in 16..128: the per-frame kernel's LDS work areas are sized for that many
 *                      tracks / detections (larger frames use a global scratch area)
 *   "chain_cus"        0 (default): the per-frame chain runs on the context's stream after the association launch; n (a multiple
 *                      of 8, <= 128): DETACHED — the chain goes to a stream of the library whose queue owns the first n compute
 *                      units of the device's CU mask (n / 8 of every XCD), ordered after the association launch; the call returns
 *                      with the caller's stream free to run its next launches.  Whoever reads d_out / d_nout (or any tracker state)
 *                      afterwards first calls ss_track_join on the stream it reads on; the library's own readers and the next
 *                      ss_track_update_group do so themselves.  The reservation is only real when every other stream of the
 *                      application is created with ss_stream_create(ctx, n, ..), i.e. without those compute units.  -1: detached onto
 *                      a plain high-priority stream (every compute unit, nothing reserved). */
int ss_set_option(ss_ctx* ctx, const char* name, int value);
/* `hip_stream` waits for the detached chain of the last ss_track_update_group (no-op without one). */
int ss_track_join(ss_ctx* ctx, void* hip_stream);
/* A non-blocking HIP stream whose queue may use every compute unit except the first `skip_cus` of the CU mask (bit i = compute
 * unit i / 8 of XCD i % 8; skip_cus == 0: a plain stream) -> *out (hipStream_t); ss_stream_destroy releases it. */
int ss_stream_create(ss_ctx* ctx, int skip_cus, void** out);
int ss_stream_destroy(ss_ctx* ctx, void* hip_stream);

/* Per-stream error flags raised on the device (capacity, infeasible); synchronous. */
int ss_check_errors(ss_ctx* ctx);

/* ---- stage entry points for known-answer tests (device pointers, natural layouts) ------------- */
int ss_feat_normalize(ss_ctx* ctx, const float* d_raw, int n, float* d_unit);
int ss_ema(ss_ctx* ctx, const float* d_smooth, const float* d_feat, int n, float* d_out);
int ss_kf_predict(ss_ctx* ctx, double* d_mean, double* d_cov, int n);
int ss_kf_update(ss_ctx* ctx, double* d_mean, double* d_cov, const double* d_z, const double* d_conf, int n);
/* a7 KalmanFilter.project with the NSA noise: d_zmean[n][4] = H x, d_S[n][4][4] = H P H^T + R(x, conf), R's deviations scaled
 * by (1 - conf); d_conf == NULL: conf = 0 (the form the gating distance uses).  The tracker runs it fused into the gate and
 * the update; this entry point exists for known-answer tests. */
int ss_kf_project(ss_ctx* ctx, const double* d_mean, const double* d_cov, const double* d_conf, int n, double* d_zmean, double* d_S);
int ss_kf_initiate(ss_ctx* ctx, const double* d_z, int n, double* d_mean, double* d_cov);
/* gallery rows natural [T][B][512] -> fragment-major [T][4][16384] used by ss_assoc_cost */
int ss_gallery_pack(ss_ctx* ctx, const float* d_gallery, int T, int B, float* d_frag);
/* fused a7+a8: cosine-gallery-min + Mahalanobis gate + blend + threshold.
 * d_counts [T] valid gallery rows; d_feats [D][512] unit rows; d_mean/d_cov predicted states;
 * d_xyah [D][4].  Outputs [T][D]: cost (f64), cosine (f32), maha (f64), gated (u8). */
int ss_assoc_cost(ss_ctx* ctx, const float* d_gallery_frag, const int* d_counts, int T,
                  const float* d_feats, int D, const double* d_mean, const double* d_cov,
                  const double* d_xyah, double* d_cost, float* d_cos, double* d_maha, uint8_t* d_gated);
int ss_iou_cost(ss_ctx* ctx, const double* d_track_tlwh, int T, const double* d_det_tlwh, int D,
                double* d_cost);
/* a9: rectangular LSAP on a [nr][nc] float64 matrix; d_row_to_col[nr] = column or -1. */
int ss_lsap(ss_ctx* ctx, const double* d_cost, int nr, int nc, int* d_row_to_col);

/* ---- inspection (synchronous; parity tests) ----------------------------------------------------
 * Track table of one stream in track-list order (arrays may be NULL). */
int ss_get_tracks(ss_ctx* ctx, int stream, int cap, int* n_tracks, int* next_id, int* track_id,
                  int* state, int* hits, int* age, int* tsu, int* class_id, float* conf,
                  double* mean, double* cov, float* smooth, int* gal_count);
/* Stage intermediates of frame `frame` of the last group (ctx created with debug != 0).
 * counts[6] = n_conf, n_cand, n_cols_b, n_dets, assignment path of the appearance stage and of the IoU stage (0 stage
 * skipped, 1 unique optimum read off the thresholded matrix, 2 LSAP); matrices are [SS_MAX_TRACKS][SS_MAX_DETS] strided. */
int ss_get_debug(ss_ctx* ctx, int stream, int frame, int* counts, float* cos, double* maha, uint8_t* gated,
                 double* cost_a, double* cost_b, int* lists /* [4][SS_MAX_TRACKS] */);
/* Gallery of one track (by position in the track list) in natural [count][512] order of slots. */
int ss_get_gallery(ss_ctx* ctx, int stream, int track_index, float* rows, int cap_rows, int* count);

/* ---- a2 / a5 glue: stateless fused NHWC-half operators around the PyTorch-ROCm convolutions -------
 * (detector / OSNet forward inside model.track, yolo_multi_model.py:41).  `stream` is a hipStream_t.
 * act: 0 none, 1 relu, 2 silu, 3 sigmoid.  Tensors are channels-last half. */
int ss_op_bias_act_f16(void* stream, void* d_x, const void* d_bias, const void* d_res, long long n_pix, int C, int act);
/* Epilogue with placement (C2f blocks): d_out[pix*out_ld + c] = act(x + bias)[c] (+ res after the activation when
 * res_after), d_out pointing at a channel slice of a wider NHWC tensor (pitch out_ld elements); channels
 * [c0, c0+cn) are also written densely to d_out2 when it is not NULL.  C, out_ld, c0, cn multiples of 8. */
int ss_op_bias_act_place_f16(void* stream, const void* d_x, const void* d_bias, const void* d_res, long long n_pix, int C,
                             int act, int res_after, void* d_out, int out_ld, void* d_out2, int c0, int cn);
/* 1x1 convolution + bias + activation (+ shortcut) in one MFMA kernel: d_out[pix*out_ld + n] =
 * act(sum_k x[pix][k] w[n][k] + bias[n] (+ res[pix][n] before, or after when res_after, the activation)); x [M][K],
 * w [N][K], res [M][N] dense NHWC half; placement arguments as ss_op_bias_act_place_f16 (multiples of 4 here).
 * K % 8 == 0, N % 8 == 0. */
int ss_op_pointwise_f16(void* stream, const void* d_x, const void* d_w, const void* d_bias, const void* d_res, long long M,
                        int K, int N, int act, int res_after, void* d_out, int out_ld, void* d_out2, int c0, int cn);
/* 3x3 / pad 1 / stride 1|2 convolution + bias + activation (+ shortcut) as an implicit GEMM on the same kernel:
 * x [B][H][W][Cin], w [N][3][3][Cin], output [B][OH][OW][N] with OH = (H-1)/stride+1; epilogue and placement
 * arguments as ss_op_pointwise_f16.  Cin % 8 == 0, N % 8 == 0. */
int ss_op_conv3x3_f16(void* stream, const void* d_x, const void* d_w, const void* d_bias, const void* d_res, int B, int H,
                      int W, int Cin, int N, int conv_stride, int act, int res_after, void* d_out, int out_ld,
                      void* d_out2, int c0, int cn);
/* A C2f bottleneck in ONE launch (nets.Bottleneck with 3x3 + 3x3, e = 1.0; reference: ultralytics' Bottleneck as the detector
 * checkpoints the reference loads define it): out = [x +] silu(conv3x3(silu(conv3x3(x, w1) + b1), w2) + b2), the intermediate kept
 * in LDS and rounded to half exactly where the two ss_op_conv3x3_f16 launches round it (the results are bit-identical to them).
 * x dense [B][H][W][C], C in {16, 32, 64, 128}; w1, w2 [C][3][3][C]; d_out points at the block's channel slice of a wider NHWC tensor
 * (out_ld halfs per pixel), d_out2 (or NULL) receives a dense [B][H][W][C] copy. */
int ss_op_bottleneck_f16(void* stream, const void* d_x, const void* d_w1, const void* d_b1, const void* d_w2, const void* d_b2,
                         int B, int H, int W, int C, int add, void* d_out, int out_ld, void* d_out2);
/* Several independent convolutions in ONE launch (the detect head's branches: nets.Detect): every entry is a 3x3 / pad 1
 * (stride 1|2) or 1x1 convolution + bias + activation on NHWC half, dense output [B][OH][OW][N]; all entries of a call have
 * the same ksize; N <= 80, n <= 8.  Weights as ss_op_conv3x3_f16 ([N][3][3][Cin]) / ss_op_pointwise_f16 ([N][Cin]). */
typedef struct ss_conv_desc {
    const void* x; const void* w; const void* bias; void* out;
    int B, H, W, Cin, N, ksize, stride, act;
} ss_conv_desc;
int ss_op_conv_group_f16(void* stream, int n, const ss_conv_desc* descs);
/* One level of the anchor-free (v8) detect head, BOTH branches and all three layers of a branch, in one launch: per branch b
 * 3x3 (Cin -> cm_b) + SiLU -> 3x3 (cm_b -> cm_b) + SiLU -> 1x1 (cm_b -> nout[b]) + bias, cm_0 = 64 (box), cm_1 = 80 (class); the
 * intermediates stay in the LDS.  d_x dense NHWC half [B][H][W][Cin], Cin in {64, 128, 256}; weights as ss_op_conv3x3_f16 /
 * ss_op_pointwise_f16 take them ([cm][3][3][Cin], [cm][3][3][cm], [nout][cm]); d_out[b] dense [B][H][W][nout[b]], nout[b] % 8 == 0,
 * <= cm_b.  Bit-identical to the three separate launches per branch (non-split-K form).  tile16: 8 x 16 tiles for Cin = 64. */
int ss_op_head_f16(void* stream, const void* d_x, const void* const* d_w1, const void* const* d_b1, const void* const* d_w2,
                   const void* const* d_b2, const void* const* d_w3, const void* const* d_b3, void* const* d_out, const int* nout,
                   int B, int H, int W, int Cin, int tile16);
/* YOLOv8 anchor-free head decode: per level l<3 the branch outputs d_box[l] [B][H][W][64] and d_cls[l] [B][H][W][nc]
 * (NHWC half, final 1x1 conv without bias; the biases are added here) -> d_pred [B][4+nc][A] float (xywh in input
 * pixels, class sigmoid), A = sum H[l]*W[l] — the tensor ss_nms reads.  H, W, strides are host int[3]. */
int ss_op_v8_decode_f16(void* stream, const void* const* d_box, const void* const* d_cls, const void* const* d_box_bias,
                        const void* const* d_cls_bias, const int* H, const int* W, const int* strides, int B, int nc,
                        float* d_pred);
/* The same with the head's third branch as extra rows 4 + nc .. 4 + nc + n_ext of the prediction [B][4 + nc + n_ext][A]: d_ext[3]
 * [B][H][W][ext_ld] half with the bias already added (the branch's last 1x1 through ss_op_pointwise_f16); ext_mode 1: keypoint
 * triplets decoded as Ultralytics Pose.kpts_decode ((2 v + cell) * stride for x and y, sigmoid for the visibility), n_ext % 3 == 0;
 * ext_mode 0: raw values (Segment's mask coefficients); ext_mode 2 (n_ext == 1): an oriented box's angle, theta = (sigmoid(v) - 1/4) pi
 * in row 4 + nc, and rows 0..3 become dist2rbox's (cx, cy, w, h): the centre's offset from the anchor turned by theta (docs/OBB.md §2).
 * cls_ld >= nc: channels per pixel of the class tensors (a one-class head
 * zero-padded to 8 so that its last 1x1 runs on ss_op_pointwise_f16).  n_ext == 0 and cls_ld == nc: ss_op_v8_decode_f16. */
int ss_op_v8_decode_ext_f16(void* stream, const void* const* d_box, const void* const* d_cls, const void* const* d_box_bias,
                            const void* const* d_cls_bias, const void* const* d_ext, int n_ext, int ext_ld, int ext_mode,
                            const int* H, const int* W, const int* strides, int B, int nc, int cls_ld, float* d_pred);
/* Depthwise 3x3 / stride 1 / pad 1 on NHWC half: y = h(act(bias + the in-image taps)), fp32 sum, one rounding; d_w9 tap-major.
 * SS_ERR_INVALID before any launch for a null tensor, C < 8 or C % 8, N, H or W < 1, act outside 0..3 (none, relu, silu, sigmoid). */
int ss_op_dwconv3x3_f16(void* stream, const void* d_x, const void* d_w9 /*[9][C]*/, const void* d_bias, void* d_y,
                        int N, int H, int W, int C, int act);
/* OSNet LightConv3x3 in one pass: y = relu(dw3x3(pw1x1(x)) + bias); w1 [C][C] (out, in), w9 [9][C], C in
 * {16,24,32}, W % 8 == 0, 18*(W+2)*PS*2 <= 65536 with PS = C rounded up to 16 (the band lives in LDS; SS_ERR_INVALID otherwise). */
int ss_op_lightconv_f16(void* stream, const void* d_x, const void* d_w1, const void* d_w9, const void* d_bias,
                        void* d_y, int N, int H, int W, int C);
/* The detector's first convolution: 3x3 / stride 2 / pad 1, 3 -> Cout in {16, 32, 48} channels, + bias + activation on
 * [B][H][W][3] half -> [B][(H-1)/2+1][W/2][Cout]; d_w_prep [4][3][Cout][16] = for conv columns c = 4n + r, per (ky, out
 * channel) the taps 3*kx+ch placed (6r + 5) % 8 halfs into a zero-padded 16-wide K window (fused.conv0_weight).  W % 128 == 0. */
int ss_op_conv0_f16(void* stream, const void* d_x, const void* d_w_prep, const void* d_bias, void* d_y, int B, int H, int W, int Cout,
                    int act);
/* Packed ReID batches: until the next call for the same stream, the OSNet-side entry points (ss_op_osnet_stem_f16,
 * ss_op_pointwise_f16, ss_op_osnet_streams_f16, ss_op_osnet_tail_f16) launched on `stream` BY THE CALLING THREAD with `batch`
 * images compute only the first *d_n of them (device int, read by the kernels; the grids stay fixed, so the launches can sit
 * in a captured graph).  d_n == NULL: off for that stream.  Per (host thread, stream): two pipelines in one process do not
 * see each other's setting.  At most 8 streams of a thread hold a setting at once (SS_ERR_CAPACITY). */
int ss_op_set_valid_images(void* stream, const int* d_n, int batch);
/* Process-wide A/B switches of the stateless operators, for measurements (default 1 each): "pw_epilogue" (16-byte vector
 * epilogue), "pw_splitk" (split-K form of small 3x3 layers), "osnet_chains" (register-resident LightConv row streams).  Sizes: "jpeg_subseq_words" (4, 8, 16 or 32), "aflink_chunk" (candidate
 * pairs per pass of the AFLink network, 1 .. 65536, default 1024). */
int ss_op_set_option(const char* name, int value);
/* OSNet stem in one pass: conv 7x7/2 pad 3 (3 -> 16) + bias + ReLU + max pool 3x3/2 pad 1 on crops [N][H][128][3]
 * half -> [N][H/4][32][16]; d_w_prep [4][7][16][32] = for conv columns c = 4n + r, per (ky, out channel) the taps 3*kx+ch
 * placed (6r + 7) % 8 halfs into a zero-padded 32-wide K window (fused.stem_weight).  W == 128, H % 16 == 0.  d_w1 != NULL:
 * also d_y1 [N][H/4][32][16] = relu(conv1x1(d_y, d_w1 [16][16]) + d_b1) — the first OSBlock's conv1, bit-identical to
 * ss_op_pointwise_f16 on d_y. */
int ss_op_osnet_stem_f16(void* stream, const void* d_x, const void* d_w_prep, const void* d_bias, void* d_y, int N, int H,
                         int W, const void* d_w1 /*[16][16] or NULL*/, const void* d_b1, void* d_y1);
/* The four LightConv3x3 chains of an OSNet block (1..4 layers deep, same input) in one launch; the intermediates stay in
 * registers (16- / 32-wide images: a wave streams the rows of a band through the layers) or in LDS:
 * d_w1 [10][C][C] = the pointwise weights of the layers of the 1-, 2-, 3-, 4-deep chain in that order; d_dwtab = their depthwise
 * taps and biases as the kernels' matrix-core operand table (ss_op_dwtab_f16 over the same ten layers, built once per set of
 * weights); d_ys[4] the chain outputs [N][H][W][C]; d_psum [4][N][bands][C] float = per-band channel sums of each output
 * (for ss_op_gate_apply_f16 / ss_op_osnet_tail_f16), bands = ss_op_osnet_streams_bands(N, H, W, C).  C in {16,24,32},
 * W % 8 == 0, 24*(2W+2)*PS*2 <= 65536 with PS = C rounded up to 16. */
int ss_op_osnet_streams_bands(int N, int H, int W, int C);
int ss_op_osnet_streams_f16(void* stream, const void* d_x, const void* d_w1, const void* d_dwtab,
                            void* const* d_ys, float* d_psum, int N, int H, int W, int C);
/* The depthwise 3x3 taps d_w9 [layers][9][C] (tap-major) and biases d_bias [layers][C] of LightConv layers as the operand table of
 * the matrix-core depthwise (csrc/ss_ops.hip DwDiag / DwTab: per layer and 16 channels six diagonal operands of 17 x 16 bytes
 * + the bias in fp32) -> d_out, ss_op_dwtab_bytes(layers, C) bytes.  C in {16, 24, 32}. */
long long ss_op_dwtab_bytes(int layers, int C);
int ss_op_dwtab_f16(void* stream, const void* d_w9, const void* d_bias, int layers, int C, void* d_out);
/* Aggregation gate with the channel means given as `parts` partial sums per (stream, image) times `scale`. */
int ss_op_gate_apply_f16(void* stream, const void* const* d_xs, int T, const void* d_w1, const void* d_b1,
                         const void* d_w2, const void* d_b2, const float* d_sums, int parts, float scale, void* d_out,
                         int N, int HW, int C, int Cr);
/* Tail of an OSNet block fused with the 1x1 convolution that follows it (nets.OSBlock.forward + the next block's conv1 or the
 * stage's ConvBR [+ AvgPool2d(2,2)]): x2 = sum_t ys[t]*gate_t (as ss_op_gate_apply_f16), o = relu(w3 x2 + b3 + idn) -> d_out
 * (may be NULL), o2 = relu(w4 o + b4) -> d_out2, 2x2-averaged first when pool != 0.  ys[4] [N][H][W][MID], idn/out
 * [N][H][W][C2], out2 [N][H][W][N2] or [N][H/2][W/2][N2]; (MID, C2, N2) in {(16,64,16|64), (24,96,24|96), (32,128,32|128)},
 * H*W % 128 == 0, 128 % W == 0; C1 == 0: d_idn is the shortcut tensor [N][H][W][C2]; C1 > 0 ((C1, C2) in {(16,64), (64,96),
 * (96,128)}, N2 == MID): d_idn is the block INPUT [N][H][W][C1] and the shortcut is its 1x1 `down` convolution d_wd [C2][C1] +
 * d_bd (no activation), computed inside; d_gates_ws: scratch for the gates (a small kernel computes them once per image).
 * Bit-identical to the separate calls. */
int ss_op_osnet_tail_f16(void* stream, const void* const* d_ys, const float* d_psum, int parts, float scale, const void* d_gw1,
                         const void* d_gb1, const void* d_gw2, const void* d_gb2, int Cr, float* d_gates_ws /*[N][4][32]*/,
                         const void* d_w3, const void* d_b3, const void* d_idn, int C1, const void* d_wd, const void* d_bd,
                         void* d_out, const void* d_w4, const void* d_b4, void* d_out2, int pool, int N, int H, int W, int MID,
                         int C2, int N2);
/* concat(nearest-neighbour x2 upsampling of d_lo [B][h][w][C1], d_hi [B][2h][2w][C2]) along channels -> d_out
 * [B][2h][2w][C1+C2] (lo_first: the upsampled tensor's channels first), one pass (the detector neck). */
int ss_op_upcat_f16(void* stream, const void* d_lo, const void* d_hi, void* d_out, int B, int h, int w, int C1, int C2, int lo_first);
/* SPPF's pooling pyramid: d_out [B][H][W][4C] = concat(x, m(x), m(m(x)), m(m(m(x)))), m = max pool 5x5 / 1 / pad 2.
 * H*W <= 1024, C % 8 == 0. */
int ss_op_sppf_pools_f16(void* stream, const void* d_x, void* d_out, int B, int H, int W, int C);
/* C2PSA attention of the v11 detectors in one launch: d_qkv [B][N][heads * 128] half, per head [q 32 | k 32 | v 64] (the fused 1x1's
 * output, N = H * W positions <= 256), d_out[b][i][h * 64 + c] = sum_j v[c][j] softmax_j(scale q_i . k_j) (+ d_pe[b][i][h * 64 + c], the
 * depthwise positional term of v, when given); fp32 scores / softmax / accumulation, probabilities rounded to half. */
int ss_op_psa_attention_f16(void* stream, const void* d_qkv, const void* d_pe, void* d_out, int B, int N, int heads, float scale);
/* OSNet's head in one launch: d_out[n][f] = relu(sum_c d_w[f][c] * mean_hw(d_x[n][.][c]) + d_bias[f]); d_x [N][HW][C] half (the last 1x1's
 * output), C == 128; the means are rounded to half before the product (as the tensor a GEMM would read), fp32 accumulation.  Honours
 * ss_op_set_valid_images. */
int ss_op_osnet_head_f16(void* stream, const void* d_x, const void* d_w, const void* d_bias, void* d_out, int N, int HW, int C, int F);
/* 2x2 / stride 2 average pooling, NHWC half (H, W even; C % 8 == 0). */
int ss_op_avgpool2_f16(void* stream, const void* d_x, void* d_y, int N, int H, int W, int C);
/* k x k max pooling (stride, pad with -inf) on NHWC half, output floor((H+2p-k)/s)+1 rows and columns alike.  SS_ERR_INVALID before any
 * launch for a null tensor, C < 8 or C % 8, k or stride < 1, N, H or W < 1, pad < 0, 2 * pad > k (a window could lie wholly in the
 * padding and yield -inf) and a window wider than the padded map (no output row or column: OH < 1 or OW < 1). */
int ss_op_maxpool_f16(void* stream, const void* d_x, void* d_y, int N, int H, int W, int C, int k, int stride, int pad);
/* OSNet unified aggregation gate: out = sum_t x_t * sigmoid(fc2(relu(fc1(mean_hw(x_t))))), T <= 4 streams. */
int ss_op_gate_sum_f16(void* stream, const void* const* d_xs, int T, const void* d_w1, const void* d_b1,
                       const void* d_w2, const void* d_b2, float* d_means_ws, void* d_out, int N, int HW, int C, int Cr);

/* ---- ReID network in fp32 (the accuracy mode, csrc/ss_ops32.hip) -------------------------------------
 * OSNet-x0.25 with fp32 activations and weights on v_mfma_f32_16x16x4_f32: what stands behind the ReID forward pass inside
 * model.track (/root/reference/yolo_multi_model.py:41, which passes no half=) when the float distances must agree with a CPU
 * fp32 network to north_star's 1e-4.  All tensors dense NHWC float; weights [out][in] row-major float; d_nvalid (optional,
 * device int): only the first *d_nvalid images are computed (packed ReID batches), the launch grids stay fixed. */
/* relu?(W x + bias (+ res)): d_x [M][K], d_w [N][K], d_out / d_res [M][N].  (K, N) one of the OSNet-x0.25 pairs. */
int ss_op32_pointwise(void* stream, const void* d_x, const void* d_w, const void* d_bias, const void* d_res, void* d_out,
                      long long M, int K, int N, int relu, const int* d_nvalid, int img_px);
/* The four LightConv chains of an OSBlock (layer = 1x1 linear, depthwise 3x3 + bias + ReLU; chains 1, 2, 3, 4 layers deep, ten
 * layers in that order): d_x1 [N][H][W][C] -> d_ys[0..3] (same shape) and d_psum [4][N][bands][C] = channel sums of each output
 * per band, bands = ss_op32_chains_bands(N, H, W, C) (1 for the row-stream kernel, which batches of >= 128 images take).  d_w1 [10][C][C], d_w9 [10][9][C] (tap-major), d_bias [10][C].
 * (C, W) in {(16, 32), (24, 16), (32, 8)}. */
int ss_op32_chains_bands(int N, int H, int W, int C);
int ss_op32_chains(void* stream, const void* d_x1, const void* d_w1, const void* d_w9, const void* d_bias, void* const* d_ys,
                   float* d_psum, int N, int H, int W, int C, const int* d_nvalid);
/* OSBlock tail + the 1x1 ConvBR after it, two launches: gate_t = sigmoid(fc2 relu(fc1 mean_t + b1) + b2) (fc1 [hidden][MID], fc2
 * [MID][hidden]) -> d_gates [4][N][MID] (caller's workspace); then x2 = sum_t gate_t * ys[t], o = relu(w3 x2 + b3 + shortcut) -> d_out
 * (may be NULL), o2 = relu(w4 o + b4) -> d_out2, 2x2-averaged when pool.  shortcut = d_xin [N][H][W][C2] (C1 == 0) or wd d_xin + bd
 * with d_xin [N][H][W][C1]. */
int ss_op32_tail(void* stream, const void* const* d_ys, const float* d_psum, int bands, const void* d_gw1, const void* d_gb1,
                 const void* d_gw2, const void* d_gb2, int hidden, float* d_gates, const void* d_w3, const void* d_b3, const void* d_xin, int C1,
                 const void* d_wd, const void* d_bd, void* d_out, const void* d_w4, const void* d_b4, void* d_out2, int pool, int N,
                 int H, int W, int MID, int C2, int N2, const int* d_nvalid);
/* Process-wide A/B switches of the fp32 operators: "chains_form" 2 (default): k32_chainsR (register-resident row stream) where it
 * applies, 1: k32_chains3 (LDS phases), 0: k32_chains everywhere; "tail_wgs" n: workgroups of the persistent tail grid (0 = default);
 * "chains_probe" (measurement only, bit 0: the row-stream kernel does not store its outputs). */
int ss_op32_set_option(const char* name, int value);
/* conv 7x7 / 2 (3 -> 16) + bias + ReLU + max pool 3x3 / 2: d_x [N][256][128][3] -> d_y [N][64][32][16]; d_w [16][148] with
 * k = (ky * 7 + kx) * 3 + c and a zero in column 147. */
int ss_op32_stem(void* stream, const void* d_x, const void* d_w, const void* d_bias, void* d_y, int N, int H, int W, const int* d_nvalid);
/* The same operator on BYTE crops [N][256][128][3] (ss_crop_norm_batch / _packed with SS_DST_HWC | SS_DST_U8): /255, mean and std are applied
 * while the rows are staged, from a table built with ss_crop_norm's own expression - outputs bit-equal to ss_op32_stem on the float crops. */
int ss_op32_stem_u8(void* stream, const void* d_x, const void* d_w, const void* d_bias, void* d_y, int N, int H, int W, const int* d_nvalid);
/* ... and with the first OSBlock's conv1 (1x1, 16 -> 16, + bias + ReLU) applied to the pooled pixels by the same launch: d_y1 [N][64][32][16] =
 * relu(W1 d_y + b1), bit-equal to ss_op32_pointwise on d_y (the stem's output is not read back).  x_u8 != 0: byte crops. */
int ss_op32_stem_conv1(void* stream, const void* d_x, int x_u8, const void* d_w, const void* d_bias, void* d_y, const void* d_w1, const void* d_b1,
                       void* d_y1, int N, int H, int W, const int* d_nvalid);
/* d_out[n][f] = relu(sum_c d_w[f][c] * mean_hw(d_x[n][.][c]) + d_bias[f]), C == 128. */
int ss_op32_head(void* stream, const void* d_x, const void* d_w, const void* d_bias, void* d_out, int N, int HW, int C, int F,
                 const int* d_nvalid);
/* The detector's convolutions in fp32 (csrc/ss_ops32.hip k32_conv / k32_conv0; the arithmetic of the detector forward behind
 * /root/reference/yolo_multi_model.py:41, :173, which passes no half=).  ss_op32_conv: d_x NHWC [N][H][W][.] with pixel stride xs
 * floats (a channel slice of a wider tensor when xs > Cin), d_w [Cout][ks][ks][Cin], d_out NHWC [N][OH][OW][.] with pixel stride os,
 * d_res (may be NULL; added AFTER the activation) with pixel stride rs; ks 1 | 3, stride 1 | 2 (1x1: 1), pad ks / 2; act 1 = SiLU,
 * 0 = none; Cin, Cout multiples of 16, pointers 16-byte aligned, strides multiples of 4.  ss_op32_conv0: the first convolution,
 * 3 -> 16 channels, 3x3, stride 2, pad 1, d_x dense NHWC [N][H][W][3], d_w [16][3][3][3]. */
int ss_op32_conv(void* stream, const void* d_x, int xs, const void* d_w, const void* d_bias, const void* d_res, int rs, void* d_out,
                 int os, int N, int H, int W, int Cin, int Cout, int ks, int stride, int act);
int ss_op32_conv0(void* stream, const void* d_x, const void* d_w, const void* d_bias, void* d_out, int os, int N, int H, int W, int act);
/* The launch ss_op32_conv makes for this problem under the current option state, computed on the host (no HIP call): *mt = 16-channel
 * output tiles per workgroup (1 | 2 | 4 | 5), *waves = waves per workgroup (4 | 8), the grid.  Same argument checks as ss_op32_conv. */
int ss_op32_conv_plan(int N, int H, int W, int Cin, int Cout, int ks, int stride, int* mt, int* waves, int* grid_x, int* grid_y);
/* cat(upsample2x_nearest(lo), hi) (lo_first != 0) or cat(hi, upsample2x_nearest(lo)) along channels in one pass (the neck's two
 * upsample + concat pairs), fp32 NHWC: d_lo [N][H/2][W/2][.] pixel stride ls, d_hi [N][H][W][.] pixel stride hs, d_out dense. */
/* YOLOv8 head decode in fp32 (DFL expectation, dist2bbox, stride scale, class sigmoid, level concat; the third branch as keypoint
 * triplets (ext_mode 1), raw (0) or an oriented box's angle (2, as ss_op_v8_decode_ext_f16)): dense NHWC float branch outputs with their bias -> d_pred [B][4 + nc + n_ext][A]. */
int ss_op32_v8_decode(void* stream, const void* const* d_box, const void* const* d_cls, const void* const* d_ext, int n_ext, int ext_ld,
                      int ext_mode, const int* H, const int* W, const int* strides, int B, int nc, int cls_ld, float* d_pred);
/* SPPF's three chained 5x5 max pools + concat in one pass, fp32: d_x NHWC [N][H][W][.] (pixel stride xs) -> d_out dense [N][H][W][4 C]. */
int ss_op32_sppf_pools(void* stream, const void* d_x, int xs, void* d_out, int N, int H, int W, int C);
int ss_op32_upcat(void* stream, const void* d_lo, int ls, int Cl, const void* d_hi, int hs, int Ch, void* d_out, int N, int H, int W, int lo_first);

/* ---- baseline JPEG frames decoded on the device (csrc/ss_jpeg.hip, docs/JPEG.md) ---------------- */
/* Accepted: SOF0, 8-bit, 1 component or 3 (YCbCr), luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, one interleaved scan, 8-bit
 * quantisation tables, any Huffman tables, restart intervals; sides 1 .. 8192.  Everything else returns SS_ERR_INVALID with the
 * cause in ss_last_error().  The pixels equal libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling) bit for bit.
 * ss_jpeg_probe: host only (no GPU, no context; the message of a refusal is in ss_last_error(NULL)): the frame's size, its
 * component count and the luma sampling factors. */
int ss_jpeg_probe(const unsigned char* data, size_t size, int* width, int* height, int* components, int* h_samp, int* v_samp);
/* Host only: the quantised coefficients as dense natural-order int16 blocks, component after component, each component's blocks
 * in raster order over its whole-MCU grid (coef_cap: capacity in values), and the four quantisation tables quant [4][64] in
 * natural order (absent tables zero).  For tests of the entropy stage. */
int ss_jpeg_coefficients(const unsigned char* data, size_t size, short* coef, size_t coef_cap, unsigned short* quant);
/* n (1 .. 64) encoded frames of one size height x width -> d_out + i * out_frame_stride, HWC uint8, BGR (rgb = 0) or RGB.  The
 * entropy stage runs inside the call on `threads` (1 .. 16) host threads; the coefficients leave in one asynchronous copy and two
 * launches on hip_stream do the rest.  The caller's buffers may be reused on return.  When a frame is refused nothing is launched
 * and the message names its index.  Not capturable (host work): never call it while hip_stream is capturing. */
int ss_jpeg_decode_batch(ss_ctx* ctx, void* hip_stream, const unsigned char* const* data, const size_t* sizes, int n, int height,
                         int width, void* d_out, long long out_frame_stride, int rgb, int threads);

/* The same call with the entropy stage on the device (docs/JPEG.md section 12): the host parses the headers and copies the scan's
 * bytes (stuffing dropped, cut at the restart markers); two more kernels decode the Huffman code.  Same arguments, same checks,
 * same pixels.  The one difference: damage that only the scan shows (a code that does not exist, a bad DC category, an index beyond
 * 63, data that ends early, bytes left over before a restart marker) is found on the device: the frame is written as if all its
 * blocks were empty and SS_ERR_INVALID, naming the image and the cause, is returned by the next ss_check_errors or by the next
 * decode call that reuses the call's staging slot (there are two), whichever comes first.  Not capturable. */
int ss_jpeg_decode_batch_device(ss_ctx* ctx, void* hip_stream, const unsigned char* const* data, const size_t* sizes, int n, int height,
                                int width, void* d_out, long long out_frame_stride, int rgb, int threads);
/* Host only (no GPU, no context): the host's share of that call for one file.  bytes: the scan without the 00 after every FF, cut
 * at the RSTn markers into segments, each padded with zeros to 4 bytes; segments: per segment {byte offset, byte length, first
 * block in scan order, blocks}; header: the 160 words of section 3 (the call's offsets zero; may be NULL).  With bytes == NULL only
 * *bytes_used (the capacity to bring) and *n_segments are written.  Header refusals and "bad restart marker" as ss_jpeg_decode_batch. */
int ss_jpeg_scan_segments(const unsigned char* data, size_t size, unsigned char* bytes, size_t bytes_cap, size_t* bytes_used, unsigned int* segments,
                          size_t seg_cap, int* n_segments, unsigned int* header);
/* The device entropy stage alone on one image, for known-answer tests: dense blocks in ss_jpeg_coefficients' layout (synchronous;
 * the stream is expanded on the host).  ss_jpeg_device_rounds: the speculation rounds each 1024-lane tile of that image took
 * (returns the number of tiles, writes at most cap). */
int ss_jpeg_device_coefficients(ss_ctx* ctx, const unsigned char* data, size_t size, short* coef, size_t coef_cap);
int ss_jpeg_device_rounds(ss_ctx* ctx, int* rounds, int cap);

/* ---- frames on the device written as baseline JPEG files (csrc/ss_jpeg_enc.hip, docs/JPEG.md "Encoding") ---- */
/* The files equal what libjpeg-turbo's defaults write (JDCT_ISLOW, the Annex K Huffman tables, JFIF header) byte for byte: YCbCr
 * with luma sampling h_samp x v_samp = 2x2 (4:2:0), 2x1 (4:2:2) or 1x1 (4:4:4), quality 1 .. 100, sides 1 .. 8192.
 * Host only: a capacity no file of that shape can exceed (negative: SS_ERR_INVALID, the cause in ss_last_error(NULL)). */
long long ss_jpeg_encode_bound(int width, int height, int h_samp, int v_samp);
/* Host only: the entropy stage and the header alone.  coef: quantised coefficients as dense natural-order int16 blocks in the
 * layout ss_jpeg_coefficients returns (blocks outside a component's real blocks are not read: the writer fills them in itself);
 * out receives the whole file (out_cap >= ss_jpeg_encode_bound), *out_size its length.  For tests of the entropy stage. */
int ss_jpeg_entropy_encode(const short* coef, int quality, int width, int height, int h_samp, int v_samp, unsigned char* out, size_t out_cap,
                           size_t* out_size);
/* n (1 .. 64) frames of one size on the device, HWC uint8, BGR (rgb = 0) or RGB, frame i at d_in + i * in_frame_stride -> n files
 * in the host buffers out[i] (out_cap[i] >= ss_jpeg_encode_bound), lengths in out_size[i].  Colour conversion, downsampling,
 * forward DCT, quantisation and the compaction of the non-zero coefficients are two launches on hip_stream; the sparse
 * coefficients come back in one copy, the call waits for it on an event of its own (no device-wide synchronisation) and Huffman-
 * codes the images on `threads` (1 .. 16) host threads.  Every argument is checked before the device is touched.  Not capturable
 * (host work, waits): never call it while hip_stream is capturing. */
int ss_jpeg_encode_batch(ss_ctx* ctx, void* hip_stream, const void* d_in, long long in_frame_stride, int n, int height, int width, int rgb,
                         int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, const size_t* out_cap, size_t* out_size);
/* The same call with the entropy stage on the device too (docs/JPEG.md section 13): same arguments, same checks, same refusals,
 * same return codes, the same files byte for byte.  Four more kernels on hip_stream turn the dense coefficients into the stuffed
 * scan (bit length per block, 64-bit scan of the lengths + write into a zeroed stream, FF count, stuffing); only the scans' own
 * bytes come back, and `threads` (1 .. 16) host threads write the headers and copy.  The call waits three times on an event of its
 * own (bit totals, FF totals, the copy); no device-wide synchronisation.  Not capturable (waits, allocations that follow the
 * totals): never call it while hip_stream is capturing. */
int ss_jpeg_encode_batch_device(ss_ctx* ctx, void* hip_stream, const void* d_in, long long in_frame_stride, int n, int height, int width,
                                int rgb, int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, const size_t* out_cap,
                                size_t* out_size);
/* For tests: the device twin of ss_jpeg_entropy_encode.  The same coefficient layout (ss_jpeg_coefficients'), uploaded as dense
 * blocks; the device entropy stage alone writes the scan, the host the header; out receives the whole file.  Synchronous, on the
 * context's stream.  Coefficients beyond the baseline categories (DC difference 11 bits, AC 10 bits), which no frame produces, are
 * refused on the host before anything is launched, with ss_jpeg_entropy_encode's message. */
int ss_jpeg_entropy_encode_device(ss_ctx* ctx, const short* coef, int quality, int width, int height, int h_samp, int v_samp,
                                  unsigned char* out, size_t out_cap, size_t* out_size);

/* ---- GSI post-processing: Gaussian-process smoothing of finished tracks (csrc/ss_gsi.hip, docs/GSI.md) ---- */
/* n_tracks (1 .. 65 536) tracks, all host pointers: track t owns rows offsets[t] .. offsets[t+1]-1 (offsets[0] = 0, non-decreasing;
 * an empty track is allowed and produces nothing) of frames (strictly increasing inside a track) and of vals [rows][4] = x1, y1, w,
 * h; len_scale[t] (finite, > 0) is its RBF length scale, alpha (finite, >= 0) is added on the kernel matrix's diagonal.  out
 * [rows][4] receives the posterior mean of each column, status[t] 0 (smoothed), 1 (a pivot was not > 0: the track's vals copied
 * through) or 2 (more than ss_gsi_max_len() rows: copied through, never sent to the device).  One upload, the launches on the
 * context's stream (one workgroup per track, the long tracks first) and one download; the call waits on an event of its own, not
 * on the device.  Every argument is checked before the context or the device is touched: a refusal returns SS_ERR_INVALID with a
 * message naming the track (ss_last_error; with ctx NULL in ss_last_error(NULL)) and leaves the context usable; a call whose
 * tracks are all empty or over the cap is settled on the host and needs no context.  The results are
 * the bits tests/gsi_ref.py computes (docs/GSI.md section 3).  Not capturable (waits, allocations that follow the call's size). */
int ss_gsi_smooth(ss_ctx* ctx, int n_tracks, const int* offsets, const int* frames, const double* vals, const double* len_scale, double alpha,
                  double* out, int* status);
/* Host only: the longest track ss_gsi_smooth sends to the device (1024). */
int ss_gsi_max_len(void);

/* ---- scoring tracks against ground truth: HOTA and CLEAR MOT (csrc/ss_mot.hip, docs/MOTEVAL.md) ---- */
/* n_pairs (1 .. 64) pairs of one ground-truth and one tracker row set, all host pointers.  Pair p owns the evaluated frames
 * frame_off[p] .. frame_off[p+1]-1 (at most 65 536); frame f owns the ground-truth rows gt_off[f] .. gt_off[f+1]-1 and the tracker
 * rows tr_off[f] .. tr_off[f+1]-1 (at most ss_mot_max_boxes() each; every offset array starts at 0 and does not decrease).  gt_ids /
 * tr_ids are the rows' dense ids, 0 .. n_gt_ids[p]-1 and 0 .. n_tr_ids[p]-1, unique within a frame; gt_boxes / tr_boxes [rows][4]
 * are x1, y1, x2, y2, finite with x2 > x1 and y2 > y1; thr in (0, 1] is CLEAR's similarity threshold.  Per ground-truth row the
 * call returns HOTA's match (hota_match: the tracker row's index within its frame or -1, hota_s: that pair's similarity or 0) and
 * CLEAR's (clear_match, clear_s); ga, unless NULL, receives the global alignment scores, per pair [n_gt_ids][n_tr_ids], pair after
 * pair.  One upload, the launches (CLEAR's walkers, one wave per pair, on a second stream of the context beside the alignment and
 * the HOTA matching) and one download; the call waits on an event of its own.  Every argument is checked before the context or the
 * device is touched: a refusal is SS_ERR_INVALID, a call over a cap (boxes a frame, pairs, frames a pair, 2^26 ground-truth id x
 * tracker id cells, 2^27 box x box cells) SS_ERR_CAPACITY, both with a message naming the pair and frame (with ctx NULL in
 * ss_last_error(NULL)), and the context stays usable.  The results are the bits tests/moteval_ref.py computes (docs/MOTEVAL.md
 * section 1).  Not capturable. */
int ss_mot_eval(ss_ctx* ctx, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_ids, const int* tr_ids,
                const double* gt_boxes, const double* tr_boxes, const int* n_gt_ids, const int* n_tr_ids, double thr,
                int* hota_match, double* hota_s, int* clear_match, double* clear_s, double* ga);
/* Host only: the most boxes one side of a frame may hold (256: the one-wave assignment solver's columns). */
int ss_mot_max_boxes(void);
/* The identity metrics of the same pairs (docs/MOTEVAL.md section 1, "Identity"): the arguments up to thr are ss_mot_eval's and are
 * checked by the same body, before the context or the device is touched, except that a pair may have at most ss_mot_max_ids()
 * ground-truth ids and as many tracker ids (more: SS_ERR_CAPACITY naming the pair) and that the box x box cap does not apply (no
 * similarity is stored).  pot[g][t] counts the frames in which both ids have a box with S >= thr - 2^-52; idtp[p] is the weight of
 * a maximum-weight one-to-one matching of pair p's ground-truth ids to its tracker ids under pot, gt_to_tr (one entry per
 * ground-truth id, pair after pair) one such matching: the dense tracker id, or -1 where the id is unmatched or its pair has
 * pot = 0.  The weight is unique; of several matchings that reach it the call returns the same one every time.  pot, unless
 * NULL, receives the counts, per pair [n_gt_ids][n_tr_ids], pair after pair.  One upload, two launches (the counts, one workgroup
 * per frame; the matching, one workgroup per pair) and one download; pot is zeroed by every call, the scratch is the context's and
 * is reused, and the call waits on an event of its own.  Not capturable. */
int ss_mot_identity(ss_ctx* ctx, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_ids, const int* tr_ids,
                    const double* gt_boxes, const double* tr_boxes, const int* n_gt_ids, const int* n_tr_ids, double thr,
                    int* idtp, int* gt_to_tr, int* pot);
/* Host only: the most ids one side of a pair may have in ss_mot_identity (4096: the workgroup-wide assignment solver's columns). */
int ss_mot_max_ids(void);

/* ---- scoring detections against ground truth: COCO AP and AR (csrc/ss_ap.hip, docs/DETEVAL.md) ---- */
/* All host pointers.  similarity 0: boxes are [rows][4] x1, y1, x2, y2 scored by IoU; 1: [rows][5] cx, cy, w, h, theta scored by
 * ProbIoU (the boxes rounded to float as csrc/ss_probiou.h takes them; no crowd rows).  A cell is one (class, image); the n_cells
 * cells come by (class, image): class k owns cells class_cell_off[k] .. class_cell_off[k+1]-1, cell c is image cell_image[c] (rising
 * inside a class; read only for messages) and owns the ground-truth rows cell_gt_off[c] .. cell_gt_off[c+1]-1 and the detections
 * cell_det_off[c] .. cell_det_off[c+1]-1, both in input order (every offset array starts at 0 and does not decrease).  gt_crowd[row]
 * is 1 for a crowd region.  iou_thrs [n_thrs] each in (0, 1], rec_thrs [n_recs] finite and not decreasing, areas [n_areas][2]
 * inclusive ranges, max_dets [n_max_dets] at least 1 and rising.  The call orders each class's detections by (score descending,
 * packed index rising; -0.0 ties 0.0), keeps the first max_dets[-1] of every cell, matches them greedily per (area range,
 * threshold) and accumulates; it returns precision [n_thrs][n_recs][n_classes][n_areas][n_max_dets] and recall
 * [n_thrs][n_classes][n_areas][n_max_dets] (-1 where a class has no ground truth that counts), and unless NULL det_rank [detections]
 * (the place of each detection in its class's order) and rec_match / rec_ignored [n_areas][n_thrs][kept detections] (both or
 * neither; the kept detections cell after cell by position: the matched ground-truth row's index within its cell or -1, and the
 * ignored bit).  One upload, the launches (a local sort, one merge pass per doubling, the matching with one wave per cell, the
 * accumulation with one workgroup per (class, area range, max_dets entry)) and one download; the call waits on an event of its own.
 * Every argument is checked before the context or the device is touched: a refusal is SS_ERR_INVALID, a call over a cap (the four
 * functions below; 16 thresholds, 8 area ranges, 4 max_dets entries, 1024 recall thresholds; 2^28 record entries) SS_ERR_CAPACITY,
 * both with a message naming the class and image (with ctx NULL in ss_last_error(NULL)), and the context stays usable.  The results
 * are the bits tests/deteval_ref.py computes (docs/DETEVAL.md section 1).  Not capturable. */
int ss_ap_eval(ss_ctx* ctx, int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_image, const int* cell_gt_off,
               const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
               int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
               const int* max_dets, double* precision, double* recall, int* det_rank, int* rec_match, int* rec_ignored);
/* Host only: the most ground-truth rows a cell may hold (1024), the most detections a cell may hold before the cut (4096), the
 * largest max_dets entry (1024) and the most detections of a call (4 194 304). */
int ss_ap_max_gts(void);
int ss_ap_max_cell_dets(void);
int ss_ap_max_keep(void);
int ss_ap_max_dets(void);

/* ---- AFLink: linking of finished tracklets by a small convolutional network (csrc/ss_aflink.hip, docs/AFLINK.md) ---- */
/* Host only: the floats of the weight blob (docs/AFLINK.md section 3), and the most tracklets a side one connected component of
 * surviving pairs may have in ss_aflink_match (256: the one-wave assignment solver's side). */
long long ss_aflink_weight_floats(void);
int ss_aflink_max_component(void);
/* The network's weights, BatchNorms folded: blob = n = ss_aflink_weight_floats() finite floats in the layout of docs/AFLINK.md
 * section 3.  Checked before the context is looked at; copied to the device, where they stay until the next call. */
int ss_aflink_set_weights(ss_ctx* ctx, const float* blob, long long n);
/* Host arrays in and out.  Tracklet t owns rows offsets[t] .. offsets[t+1]-1 (at least one; offsets[0] == 0) of feats [rows][3] =
 * frame (an integer, strictly increasing inside a tracklet), x1, y1.  Tracklet i (the earlier) and j (the later) are a candidate
 * if i != j, thr_t0 <= first frame of j - last frame of i < thr_t1 and sqrt(dx dx + dy dy) <= thr_s from i's last (x1, y1) to j's
 * first (f64, no fma), and i starts first: (first frame of i, i) < (first frame of j, j), so the links of any matching of the candidates
 * have no cycle.  *n_pairs receives the number of candidates.  cap == 0: nothing else is written (the caller sizes its arrays
 * by the count and calls again).  cap >= the count: pair_i, pair_j (row-major: i rising, then j rising) and cost [count] = 1 -
 * p[1] of the network for every candidate; inputs, when not NULL, receives the normalised network inputs [count][2][30][3].
 * 0 < cap < the count: SS_ERR_CAPACITY, the message names the count (a sized call makes room for min(cap, n (n - 1) / 2) candidates before it counts).  Every argument is checked before the context or the device
 * is looked at (SS_ERR_INVALID, also with a NULL context); without weights SS_ERR_INVALID.  The candidates pass the network in
 * chunks (ss_op_set_option "aflink_chunk", default 1024) through scratch that belongs to the context and grows on demand.  Two
 * identical calls give the same bytes.  Not capturable (waits, allocations that follow the call's size). */
int ss_aflink_cost(ss_ctx* ctx, int n_tracklets, const int* offsets, const double* feats, int thr_t0, int thr_t1, double thr_s, long long cap,
                   int* pair_i, int* pair_j, double* cost, float* inputs, long long* n_pairs);
/* The matching of the pairs whose cost < thr_p (a cost equal to thr_p is left out): maximum cardinality, then minimum cost sum,
 * solved per connected component of the surviving pairs by the one-wave solver in SciPy's scan order on the component's matrix
 * (1e5 where a cell is no surviving pair), one launch for all components.  pair_i / pair_j [n_pairs] must be row-major and
 * distinct, as ss_aflink_cost gives them; the costs are the caller's.  successor [n_tracklets] receives per tracklet the tracklet
 * linked behind it, or -1.  A component with more than ss_aflink_max_component() tracklets a side is SS_ERR_CAPACITY (the message
 * names its size; successor is all -1, nothing is truncated).  Pairs a caller made up may link in a circle; aflink.merge refuses
 * such a successor array.  Arguments are checked first, as above. */
int ss_aflink_match(ss_ctx* ctx, int n_tracklets, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost, double thr_p,
                    int* successor);

/* ---- analytics behind the trackers: line crossings, zones, dwell and a heat map (csrc/ss_zone.hip, docs/ZONES.md) ---- */
/* Host only: the caps (16 lines, 16 zones, 32 vertices a zone, 1024 live tracks a stream). */
int ss_zone_max_lines(void);
int ss_zone_max_zones(void);
int ss_zone_max_vertices(void);
int ss_zone_max_live(void);
typedef struct ss_zone_config {
    int anchor;                  /* 1     0: centre of the box, 1: middle of its bottom edge                   */
    int max_gap;                 /* 30    a track unseen for more frames than this has lost its state (1..32)  */
    int n_classes;               /* 80    classes the line counts are kept for (1..128)                        */
    int heat;                    /* 0     0: off, 1: +1 at the anchor's cell, 2: +1 in every cell under the box */
    int heat_cell_log2;          /* 3     a heat cell is 2^k pixels a side (0..6)                              */
    int frame_h, frame_w;        /*       frame size in pixels (read when heat is on)                          */
} ss_zone_config;
/* The state is hung off an existing context and shared by its streams; a second call replaces it.  lines [n_lines][4] = ax, ay, bx,
 * by (directed a -> b); zone q owns the vertices poly_off[q] .. poly_off[q+1]-1 of poly_xy [..][2] (poly_off[0] == 0, 3 to 32 each);
 * coordinates are integer pixels within +-32767.  With heat on the grid is ceil(frame_h / cell) x ceil(frame_w / cell), at most
 * 65 536 cells.  Every argument is checked before the context or the device is touched: a refusal returns SS_ERR_INVALID with a
 * message naming the line or zone (ss_last_error; with ctx NULL in ss_last_error(NULL)). */
int ss_zone_create(ss_ctx* ctx, const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy, const int* poly_off, int n_zones);
int ss_zone_destroy(ss_ctx* ctx);
int ss_zone_reset(ss_ctx* ctx, int stream);                /* stream < 0: all streams; tables, totals, heat, frame counter and error word */
/* A group of n_frames (1..32) frames of every stream in ONE launch, the frames in order: d_rows [n_frames][n_streams][SS_MAX_TRACKS][8]
 * and d_nrows [n_frames][n_streams] as every tracker's update_group leaves them (16-byte aligned; a count above SS_MAX_TRACKS is
 * read as SS_MAX_TRACKS; a NEGATIVE count: the stream sits that frame out, its frame counter does not move and nothing is written
 * for it).  Outputs, each skipped when NULL: d_events [F][S][R] u32 (bit l: line l crossed inward, bit 16+l outward), d_inside
 * [F][S][R] u32 zone bits, d_dwell [F][S][R] i32, d_line_totals [F][S][16][2] i32 cumulative in / out, d_occupancy [F][S][16] i32,
 * d_heat_frames [F][S][gh][gw] i32 the grid after each frame, d_heat_max [F][S] i32 its maximum (R = SS_MAX_TRACKS).  Asynchronous
 * on the context's stream, capturable.  With ss_zone_max_live() live tracks a new id counts as a first appearance, leaves no
 * state, and SS_ERR_CAPACITY is reported by ss_check_errors until ss_zone_reset.  The bits are those of tests/zones_ref.py. */
int ss_zone_update_group(ss_ctx* ctx, int n_frames, const float* d_rows, const int* d_nrows, uint32_t* d_events, uint32_t* d_inside,
                         int* d_dwell, int* d_line_totals, int* d_occupancy, int* d_heat_frames, int* d_heat_max);
/* Synchronous, host arrays, any may be NULL: frames seen, line_class [16][2][n_classes], line_totals [16][2] (in, out), per zone
 * entries, exits, the dwell frames summed over the exits, the longest dwell among them, the peak occupancy; the heat grid's maximum. */
int ss_zone_get_totals(ss_ctx* ctx, int stream, int* frames, int* line_class, int* line_totals, int* zone_entries, int* zone_exits,
                       long long* zone_dwell_sum, int* zone_longest, int* zone_peak, int* heat_max);
/* Synchronous: the stream's cumulative grid into grid [gh][gw] (cap: the ints it holds; gh, gw receive the grid's shape, also when cap is 0). */
int ss_zone_get_heat(ss_ctx* ctx, int stream, int* grid, int cap, int* gh, int* gw);
/* Where the stream's cumulative grid and its maximum live on the device (for ss_zone_heat_blend with heat_frame_stride 0). */
int ss_zone_heat_device(ss_ctx* ctx, int stream, void** d_heat, void** d_max);
/* The blend's colour table: 256 x 3 bytes, B G R. */
int ss_zone_set_colormap(ss_ctx* ctx, const uint8_t* bgr_256x3);
/* In place over batch BGR frames laid out as ss_overlay's: per pixel v = heat[y >> k][x >> k] of frame b's grid at d_heat + b *
 * heat_frame_stride ints (0: one grid for all), m = max(d_max[b * max_stride], 1); v <= 0 leaves the pixel alone, otherwise
 * t = (min(v, m) * 255 + m / 2) / m, col = table[t] and every channel becomes (pix * (256 - alpha) + col * alpha + 128) >> 8
 * (alpha 0..256).  Asynchronous on hip_stream.  The arguments are checked before the context (SS_ERR_INVALID, also with ctx NULL);
 * h, w must be the zone state's. */
int ss_zone_heat_blend(ss_ctx* ctx, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
                       const int* d_heat, long long heat_frame_stride, const int* d_max, int max_stride, int alpha);

/* ---- redaction of regions of resident frames before they are saved: blur, pixelate, fill (csrc/ss_redact.hip, docs/REDACT.md; the
 * bytes are those of tests/redact_ref.py) ---- */
/* Host only: the caps (1024 regions a frame, 4096 vertices a polygon, blur radius 31) and the scratch a call needs, in bytes (sized
 * for every 64 x 32 tile of every frame; negative: batch outside 1..65535 or a side outside 1..8192). */
int ss_redact_max_regions(void);
int ss_redact_max_vertices(void);
int ss_redact_max_radius(void);
long long ss_redact_scratch_bytes(int batch, int h, int w);
/* In place over batch BGR frames laid out as ss_overlay's.  d_regions: 8 ints a region {type, x0, y0, x1, y1, vertex offset, vertices,
 * 0}; frame b owns d_region_off[b] .. d_region_off[b+1] (at most ss_redact_max_regions() of them are read):
 *   type 0 rectangle, inclusive corners in any order, clipped to the frame      type 1 the ellipse inscribed in that clipped rectangle
 *   type 2 polygon: the even-odd interior by ss_overlay's rule united with its 2-pixel-thick outline; (x0,y0)-(x1,y1) is the bounding
 *          box of its vertices, d_verts + 2 * offset its (x, y) pairs, each within -8192 .. 16383; fewer than 3 vertices cover nothing.
 * effect 0: (2 strength + 1)^2 box mean, strength 1 .. ss_redact_max_radius(), reflect-101 borders by repeated reflection;
 * effect 1: mosaic of strength x strength cells (4, 8, 16 or 32) aligned to the frame's origin, each the rounded mean of its pixels
 * inside the frame; effect 2: fill_bgr (B | G << 8 | R << 16).  Every output pixel is a function of the untouched frame alone:
 * overlap, order and splitting of regions change no byte; pixels outside every region and row padding are not written.  d_scratch: 16-byte
 * aligned, scratch_bytes >= ss_redact_scratch_bytes(batch, h, w), owned by the call until it has run.  Asynchronous on hip_stream,
 * capturable, no host dependency.  Every argument is checked before the context is touched (SS_ERR_INVALID, also with ctx NULL). */
int ss_redact(ss_ctx* ctx, void* hip_stream, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
              const int* d_regions, const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, void* d_scratch,
              long long scratch_bytes);

/* ---- identities across cameras: a descriptor per track id kept beside a tracker, and the linking of the cameras' tracklets after
 * the run (csrc/ss_mtmc.hip, docs/MTMC.md; the bits are those of tests/mtmc_ref.py) ---- */
/* Host only: the most ids a bank may be made for (65 536) and the most tracklets of one ss_mtmc_link (2048). */
int ss_bank_max_ids(void);
int ss_mtmc_max_tracklets(void);
/* The bank is hung off an existing context, one table per stream of it: per track id 1..max_ids the f64 sum of the unit features of
 * its rows, their count, first and last frame and the last class (4 KiB an id and stream).  A second call replaces it.  Every
 * argument of every ss_bank_* entry is checked before the device is touched (SS_ERR_INVALID, also with ctx NULL). */
int ss_bank_create(ss_ctx* ctx, int max_ids);
int ss_bank_destroy(ss_ctx* ctx);
int ss_bank_reset(ss_ctx* ctx, int stream);                /* stream < 0: all streams; sums, counts, frame counter and error word */
/* A group of n_frames (1..32) frames of every stream in ONE launch, the frames in order: d_rows [n_frames][n_streams][SS_MAX_TRACKS][8]
 * and d_nrows [n_frames][n_streams] as every tracker's update_group leaves them, d_feats [n_frames][n_streams][SS_MAX_DETS][512] the
 * raw features that tracker call read; all read in place.  A row contributes when 0 <= det_idx < SS_MAX_DETS, 1 <= track_id <=
 * max_ids and its feature's squared norm is positive and finite; a NEGATIVE count: the stream sits that frame out and its frame
 * counter does not move.  Asynchronous on the context's stream (behind a detached tracker chain), capturable, no allocation.  An id
 * above max_ids contributes nothing and SS_ERR_CAPACITY is reported by ss_check_errors until ss_bank_reset. */
int ss_bank_update_group(ss_ctx* ctx, int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats);
/* Synchronous, host arrays: the ids of the stream with a count > 0 in rising order, *n of them; ids, counts, first, last, cls [cap]
 * and desc [cap][512], desc = (float)(sum / |sum|).  cap 0: only *n is written (the arrays may be NULL); a cap below *n is
 * SS_ERR_INVALID. */
int ss_bank_get(ss_ctx* ctx, int stream, int cap, int* n, int* ids, int* counts, int* first, int* last, int* cls, float* desc);
/* Links T tracklets (host arrays: desc [T][512] unit descriptors, camera index, first and last frame, row count, each [T]):
 * D[i][j] = 1 - desc_i . desc_j in f32 for i < j; i and j conflict when they share a camera and their [first, last] overlap, or when
 * either has fewer than min_rows rows; then average-linkage clustering in f64, merging the smallest (d, a, b) with d < thr among the
 * pairs without a conflict until none is left.  global_id [T]: 1.. in rising order of each cluster's smallest tracklet; merges
 * [T - 1][3] = (a, b, height) in order, *n_merges of them; dist_out (may be NULL) [T][T]: D, zero where i >= j.  T above
 * ss_mtmc_max_tracklets() is SS_ERR_CAPACITY, the message naming T, before anything runs.  Synchronous, not capturable, scratch of the
 * context that grows on demand; two identical calls give the same bytes. */
int ss_mtmc_link(ss_ctx* ctx, int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr, int min_rows,
                 int* global_id, double* merges, int* n_merges, float* dist_out);

/* ---- sliced inference: the frame cut into overlapping tiles before the detector, the tiles' rows merged after it (csrc/ss_slice.hip,
 * docs/SLICE.md; the bits are those of tests/slice_ref.py) ---- */
/* Host only: the caps (64 tiles a frame, the full-frame tile included; 8192 candidates a frame = tiles x rows_per_tile). */
int ss_slice_max_tiles(void);
int ss_slice_max_candidates(void);
/* The state is hung off an existing context; a second call replaces it.  h_tiles [n_tiles][8] = {x0, y0, tile_w, tile_h, new_w, new_h,
 * pad_left, pad_top}: the tile's window in the frame_h x frame_w frame, the size it is resized to and where that lands in the
 * canvas_h x canvas_w detector input all tiles share.  rows_per_tile: rows a tile's NMS may keep (the merge reads that many at most);
 * n_extra: columns behind the six of a row; the first n_kpt triples of them are keypoints (x, y, conf), which the merge re-expresses as
 * ((k - pad_t) / gain_t + origin) * kpt_gain + kpt_pad, the whole frame's letterbox.  Every argument is checked before the context or
 * the device is touched (SS_ERR_INVALID and a message naming the tile, also with ctx NULL). */
int ss_slice_config(ss_ctx* ctx, const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile,
                    int n_extra, int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y);
/* d_geom [batch][n_tiles][5]: ss_nms_batch's geometry rows {gain, pad_x, pad_y, tile_w, tile_h} of the configured tiles, repeated per
 * frame (image = frame * n_tiles + tile).  Synchronous; not inside a capture. */
int ss_slice_nms_geom(ss_ctx* ctx, float* d_geom, int batch);
/* ss_letterbox_batch for every tile of `batch` resident frames in ONE launch: frame b at d_src + b * src_batch_stride bytes (frame_h x
 * frame_w BGR u8, row_stride bytes a row), output image b * n_tiles + t at d_dst + (b * n_tiles + t) * 3 * canvas_h * canvas_w elements,
 * dst_flags as ss_letterbox's.  A tile's image equals ss_letterbox_batch on a cropped copy of the tile, bit for bit.  Asynchronous on
 * the context's stream, capturable; batch * n_tiles <= 65535. */
int ss_slice_letterbox_batch(ss_ctx* ctx, const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, void* d_dst, int dst_flags,
                             int pad_value);
/* The tiles' NMS rows of `batch` frames into one row list per frame.  Tile t of frame b: rows at d_rows + b * frame_stride + t *
 * tile_stride floats (row_stride floats a row, tile pixels, descending score), count d_counts[b * n_tiles + t] (read as
 * min(max(count, 0), rows_per_tile)).  mode 0: greedy NMS across tiles, 1: SAHI's GREEDYNMM (a kept box grows to the union of the
 * candidates it removed while metric(box so far, candidate) > thr); metric 0: IoU, 1: intersection over the smaller area; a candidate
 * is removed when an earlier kept one matches it with metric >= thr (and, unless agnostic, the same class column).  Outputs: up to
 * out_cap rows a frame in frame pixels at d_out + b * out_frame_stride (out_row_stride floats a row), d_out_count[b], and per row the
 * source index tile * rows_per_tile + row at d_out_src + b * src_frame_stride.  Asynchronous on the context's stream, capturable; the
 * first call with a larger batch than any before grows the workspace and must not be inside a capture. */
int ss_slice_merge(ss_ctx* ctx, const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride, long long frame_stride,
                   int mode, int metric, float thr, int agnostic, int out_cap, float* d_out, int out_row_stride, long long out_frame_stride,
                   int* d_out_count, int* d_out_src, long long src_frame_stride);

/* ---- profiling support ----------------------------------------------------------------------- */
/* Mean duration (ms) of the association (cosine gallery) kernel over the launches since the last
 * call, measured with HIP events on the context stream; also returns the launch count. */
int ss_assoc_timing(ss_ctx* ctx, int enable, float* mean_ms, int* launches);
/* The individual durations (ms, launch order) behind the mean the LAST ss_assoc_timing call returned: up to `cap` values into
 * out_ms, *n = how many there were.  For distributions (p50 / p95 / max) instead of a mean. */
int ss_assoc_timing_values(ss_ctx* ctx, float* out_ms, int cap, int* n);
/* The same kernel timed from inside: first workgroup start -> last workgroup end (100 MHz wall clock, written by the
 * kernel itself), i.e. without the time a dispatch waits for compute units behind other streams' kernels.  Returns
 * the mean over the launches since the last call (microseconds) and re-arms / disarms the stamps. */
int ss_assoc_inkernel_timing(ss_ctx* ctx, int enable, double* mean_us, int* launches);
/* enable = 2 above also records, for every workgroup of the last launch, the stamps of its first work item: [0] kernel
 * entry, [1] work record read, [2] first gallery pieces + detection operand arrived, [3] operand staged in LDS, [4..11]
 * k-segments 0..7 done, [12] results written.  out: [n_workgroups][16] 100 MHz ticks.  Profiling aid. */
int ss_assoc_timeline(ss_ctx* ctx, long long* out, int n_workgroups);

#ifdef __cplusplus
}
#endif
#endif
