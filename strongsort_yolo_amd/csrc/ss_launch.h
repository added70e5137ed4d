// ss_launch.h — what ss_api.hip calls in the other translation units, declared once with the definitions' parameter names:
// the kernel launchers and the host-side state of the stages and the tracker families.  ss_api.hip and every file that defines one of
// these include it, so each definition is compiled next to its declaration.  C++ linkage: none of this is part of the C ABI.
// (What those states are made of, the owning buffers and the HIP check of the *_impl functions, is in ss_host.h.)
#pragma once
#include <string>
#include <vector>
#include "ss_common.h"
#include "ss_host.h"

// ---- ss_track.hip: StrongSORT tracker chain and the stage kernels behind the known-answer entry points
void   ss_step_kernel_attr();
size_t ss_lsap_lds_bytes();
size_t ss_frame_lds_bytes(int cap_cost, int cap_t, int cap_d);
void ss_launch_group_head(const SSDev& dev, const SSParams& prm, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev_assoc);
void ss_launch_group_chain(const SSDev& dev, const SSParams& prm, hipStream_t st);
void ss_launch_normalize(const float* raw, int n, float* unit, hipStream_t st);
void ss_launch_ema(const float* s, const float* f, int n, float a, float b, float* o, hipStream_t st);
void ss_launch_kf(int op, double* mean, double* cov, const double* z, const double* conf, int n, double wp, double wv, hipStream_t st);
void ss_launch_project(const double* mean, const double* cov, const double* conf, int n, double wp, double* zmean, double* S, hipStream_t st);
void ss_launch_pack(const float* nat, int T, int B, float* frag, hipStream_t st);
void ss_launch_assoc(const float* gal_frag, const int* counts, int T, const float* feats, int D, const double* mean, const double* cov,
                     const double* xyah, const SSParams& prm, float* feat_frag_scratch, float* part_min_scratch, double* cost, float* cosd,
                     double* maha, uint8_t* gated, hipStream_t st);
void ss_launch_iou(const double* t, int T, const double* d, int D, double md, double* cost, hipStream_t st);
void ss_launch_lsap(const double* cost, int nr, int nc, int* r2c, double* scratch, int* err, hipStream_t st);

// ---- ss_front.hip: letterbox, NMS, ReID crops, result hand-over
int    ss_front_init();
extern __attribute__((visibility("hidden"))) int ss_nms_fused;     // a variable's name is not mangled: hidden keeps it out of the exported ss_* names
size_t ss_nms_workspace_bytes();
int*   ss_nms_error_flag(void* ws, int unit);
void ss_launch_letterbox(const uint8_t* src, int batch, long long src_batch_stride, int h, int w, int stride, void* dst, int flags, int out_h,
                         int out_w, int new_h, int new_w, int pad_top, int pad_left, int pad_value, hipStream_t st);
int  ss_launch_nms(const float* pred, int batch, long long pred_stride, int N, int nc, int n_extra, float conf, float iou, int agnostic,
                   float max_wh, int max_det, float gain, float pad_x, float pad_y, float w0, float h0, const float* geom, float* rows,
                   int row_stride, long long rows_batch_stride, int* keep, long long keep_batch_stride, int* count, void* ws, size_t ws_bytes,
                   unsigned long long cm0, unsigned long long cm1, hipStream_t st);
int  ss_launch_nms_obb(const float* pred, int batch, long long pred_stride, int N, int nc, float conf, float iou, int agnostic, int max_det,
                       const float* geom, float* rows, int row_stride, long long rows_batch_stride, int* keep, long long keep_batch_stride,
                       int* count, void* ws, size_t ws_bytes, unsigned long long cm0, unsigned long long cm1, hipStream_t st);
void ss_launch_probiou(const float* a, int n, const float* b, int m, double* out, hipStream_t st);
void ss_launch_crop(const uint8_t* frame, int batch, long long frame_batch_stride, int h, int w, int stride, const float* dets, int det_stride,
                    long long dets_batch_stride, int n, const int* d_count, void* out, int flags, hipStream_t st, const int* d_off);
void ss_launch_crop_offsets(const int* counts, int batch, int n, int* off, hipStream_t st);
void ss_launch_unpack_feats(const void* emb, int half, const int* off, const int* counts, int batch, int n, float* feats,
                            long long feats_img_stride, hipStream_t st);
void ss_launch_pack_results(const int* n_dets, const float* dets, int det_ld, int det_cap, const int* n_out, const float* out, int out_ld,
                            int out_cap, float* dst, hipStream_t st);

// ---- ss_overlay.hip, ss_cmc.hip, ss_gmc.hip, ss_mask.hip, ss_byte.hip, ss_native.hip
void ss_launch_overlay(uint8_t* frames, int batch, long long frame_stride, int h, int w, int row_stride, const void* prims,
                       const int* prim_off, const uint8_t* chars, const uint8_t* font, hipStream_t st);
void ss_launch_cmc(const uint8_t* frames, int n_images, long long frame_stride, int h, int w, int row_stride, uint8_t* smalls,
                   long long img_stride, int S, int n_frames, int hs, int ws, int max_iter, double eps, int* prev_valid,
                   const int* n_valid, double* warps, hipStream_t st);
void ss_launch_gmc_sparse(const SSGmcDev& g, const uint8_t* frames, int n_frames, long long frame_stride, int row_stride,
                          const int* n_valid, double* warps, hipStream_t st);
int  ss_mask_max_words();
void ss_launch_mask_assemble(const void* proto, int f16, long long proto_fs, int nm, int mh, int mw, const float* dets, long long dets_fs,
                             int ld, int coef_off, const int* counts, int S, int R, const float* geom, long long geom_fs, int ih, int iw,
                             uint32_t* bits, long long bits_fs, hipStream_t st);
void ss_launch_mask_outline(const uint32_t* bits, long long bits_fs, const int* counts, int S, int R, int ih, int iw, int cap, int* pts,
                            long long pts_fs, int* npts, long long npts_fs, uint32_t* copy, long long copy_fs, int* scratch, int slots,
                            hipStream_t st);
void ss_launch_byte_group(const SSByteDev& b, int F, const float* dets, const int* ndets, const float* feats, float* out, int* nout,
                          hipStream_t st);
void ss_launch_byte_group_kpts(const SSByteDev& b, int F, const float* dets, const int* ndets, const float* kpts, long long stride, int off,
                               const float* geom, float* out, int* nout, hipStream_t st);
void ss_launch_byte_group_obb(const SSByteDev& b, int F, const float* dets, const int* ndets, float* out, float* rbox, int* nout, hipStream_t st);
void ss_launch_ocsort_group(const SSOcDev& o, int F, const float* dets, const int* ndets, float* out, int* nout, hipStream_t st);
void ss_launch_deepoc_group(const SSDeepOcDev& x, int F, const float* dets, const int* ndets, const float* feats, float* out, int* nout,
                            hipStream_t st);
void ss_launch_hybrid_group(const SSHyDev& o, int F, const float* dets, const int* ndets, float* out, int* nout, hipStream_t st);
void ss_launch_native_feats(int n_img, int half, const void* const* p, const long long* img_stride, const long long* row_stride,
                            const long long* pix_stride, const int* channels, const int* height, const int* width, int s,
                            const int* keep, long long keep_stride, const int* counts, float* out, hipStream_t st);

// ---- the tracker families' states of a context: BYTE (ss_byte.hip), OC-SORT (ss_ocsort.hip), Deep OC-SORT (ss_deepoc.hip).
// `entry` is the C entry's name (`who`: with its ": ").  create replaces a state (the caller has drained the stream) and leaves none on
// failure; create, reset and every get synchronise.  SsWarpFlags: the context's per-stream flags of the two warp estimators (G-04).
struct SsWarpFlags { int *cmc, *gmc; };
int  ss_tracker_pending_impl(const int* d_err, int S, hipStream_t st, const char* family, std::string& err);
struct SSByte;
const SSByteDev& ss_byte_dev(const SSByte* b);
int  ss_byte_create_check_impl(const ss_byte_config* cfg, std::string& err);
int  ss_byte_create_impl(SSByte** pb, hipStream_t st, SsWarpFlags wf, int n_streams, const ss_byte_config* cfg, std::string& err);
int  ss_byte_reset_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int stream, std::string& err);
int  ss_byte_set_reid_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, double proximity_thresh, double appearance_thresh, double alpha, std::string& err);
int  ss_byte_set_pose_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, int n_kpt, const double* sigmas, double proximity_thresh, double pose_thresh,
                           double vis_thresh, int min_common, std::string& err);
int  ss_byte_set_obb_impl(SSByte* B, hipStream_t st, SsWarpFlags wf, int on, std::string& err);
int  ss_byte_set_gmc_impl(SSByte* B, const double* d_warps, std::string& err);
int  ss_byte_pending_impl(SSByte* B, hipStream_t st, std::string& err);
// what a BYTE read-back fills: each NULL or room for cap rows (the counts: one int, written also when cap is too small)
struct SsByteRows {
    int *n_tracked = nullptr, *n_lost = nullptr, *next_id = nullptr, *frame_id = nullptr;
    int *track_id = nullptr, *state = nullptr, *activated = nullptr;
    double* mean = nullptr;
    float *smooth = nullptr, *angles = nullptr;         // ReID's, oriented boxes': refused when the mode was never switched on, as are
    double* offsets = nullptr; unsigned* visible = nullptr; bool pose = false;      // the keypoints' (pose: their entry; it may ask for neither)
};
int  ss_byte_get_impl(SSByte* B, hipStream_t st, const char* entry, int s, int cap, const SsByteRows& r, std::string& err);
int  ss_byte_get_det_keypoints_impl(SSByte* B, hipStream_t st, int frame, int s, float* xy, unsigned* visible, std::string& err);
void ss_byte_free(SSByte* b);
struct SSOc;
struct SSDeepOc;
const SSOcDev& ss_ocsort_dev(const SSOc* o);            // the launch arguments: for the launchers, the entries' mode checks and the
const SSDeepOcDev& ss_deepoc_dev(const SSDeepOc* d);    // ss_oc_* functions, which serve both OC-SORT families
int  ss_oc_carve_impl(SSOcDev& o, SsBuf<SS_DEVICE>& buf, hipStream_t st, const char* who, std::string& err);
int  ss_oc_reset_impl(const SSOcDev& o, hipStream_t st, int stream, const char* who, std::string& err);
int  ss_oc_get_tracks_impl(const SSOcDev& o, hipStream_t st, const char* entry, int s, int cap, int* n_tracks, int* next_id, int* frame_count,
                           int* track_id, int* age, int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P,
                           float* last_obs, double* velocity, std::vector<int>* slots, std::string& err);
int  ss_ocsort_create_check_impl(const ss_ocsort_config* cfg, std::string& err);
int  ss_ocsort_create_impl(SSOc** po, hipStream_t st, int S, const ss_ocsort_config* cfg, std::string& err);
int  ss_ocsort_pending_impl(SSOc* o, hipStream_t st, std::string& err);
void ss_ocsort_free(SSOc* o);
int  ss_deepoc_create_check_impl(const ss_deepoc_config* cfg, std::string& err);
int  ss_deepoc_create_impl(SSDeepOc** pd, hipStream_t st, SsWarpFlags wf, int S, const ss_deepoc_config* cfg, std::string& err);
int  ss_deepoc_reset_impl(SSDeepOc* d, hipStream_t st, SsWarpFlags wf, int stream, std::string& err);
void ss_deepoc_set_gmc_impl(SSDeepOc* d, const double* d_warps);
int  ss_deepoc_get_features_impl(SSDeepOc* d, hipStream_t st, int s, int cap, float* emb, std::string& err);
int  ss_deepoc_pending_impl(SSDeepOc* d, hipStream_t st, std::string& err);
void ss_deepoc_free(SSDeepOc* d);
struct SSHybrid;                                        // Hybrid-SORT (ss_hybrid.hip, docs/HYBRIDSORT.md)
const SSHyDev& ss_hybrid_dev(const SSHybrid* h);
int  ss_hybrid_create_check_impl(const ss_hybridsort_config* cfg, std::string& err);
int  ss_hybrid_create_impl(SSHybrid** ph, hipStream_t st, int S, const ss_hybridsort_config* cfg, std::string& err);
int  ss_hybrid_reset_impl(SSHybrid* h, hipStream_t st, int stream, std::string& err);
int  ss_hybrid_get_tracks_impl(SSHybrid* h, hipStream_t st, int s, int cap, int* n_tracks, int* next_id, int* frame_count, int* track_id,
                               int* age, int* time_since_update, int* hits, int* hit_streak, int* frozen, double* x, double* P,
                               float* last_obs, double* velocity, float* conf, float* conf_prev, std::string& err);
int  ss_hybrid_pending_impl(SSHybrid* h, hipStream_t st, std::string& err);
void ss_hybrid_free(SSHybrid* h);

// ---- ss_jpeg.hip: decoder state of a context (created on first use)
struct SSJpeg;
int  ss_jpeg_probe_impl(const unsigned char* data, size_t size, int* width, int* height, int* components, int* h_samp, int* v_samp, std::string& err);
int  ss_jpeg_coefficients_impl(const unsigned char* data, size_t size, short* coef, size_t coef_cap, unsigned short* quant, std::string& err);
int  ss_jpeg_decode_impl(SSJpeg** state, hipStream_t stream, const unsigned char* const* data, const size_t* sizes, int n, int height, int width,
                         void* d_out, long long out_frame_stride, int rgb, int threads, std::string& err);
void ss_jpeg_free(SSJpeg* j);
int  ss_jpeg_scan_segments_impl(const unsigned char* data, size_t size, unsigned char* bytes, size_t bytes_cap, size_t* bytes_used,
                                unsigned int* segments, size_t seg_cap, int* n_segments, unsigned int* header, std::string& err);
int  ss_jpeg_decode_device_impl(SSJpeg** state, hipStream_t stream, const unsigned char* const* data, const size_t* sizes, int n, int height,
                                int width, void* d_out, long long out_frame_stride, int rgb, int threads, short* coef, size_t coef_cap,
                                std::string& err);
int  ss_jpeg_pending_impl(SSJpeg* j, std::string& err);
int  ss_jpeg_device_rounds_impl(SSJpeg* j, int* rounds, int cap);

// ---- ss_jpeg_enc.hip: encoder state of a context
struct SSJpegEnc;
size_t ss_jpeg_encode_bound_impl(int width, int height, int h_samp, int v_samp);
int  ss_jpeg_entropy_encode_impl(const short* coef, int quality, int width, int height, int h_samp, int v_samp, unsigned char* out,
                                 size_t* out_size, std::string& err);
int  ss_jpeg_encode_impl(SSJpegEnc** state, hipStream_t stream, const void* d_in, long long in_frame_stride, int n, int height, int width,
                         int rgb, int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, size_t* out_size, std::string& err);
int  ss_jpeg_encode_device_impl(SSJpegEnc** state, hipStream_t stream, const void* d_in, long long in_frame_stride, int n, int height, int width,
                                int rgb, int quality, int h_samp, int v_samp, int threads, unsigned char* const* out, size_t* out_size,
                                std::string& err);
int  ss_jpeg_entropy_encode_device_impl(SSJpegEnc** state, hipStream_t stream, const short* coef, int quality, int width, int height, int h_samp,
                                        int v_samp, unsigned char* out, size_t* out_size, std::string& err);
void ss_jpeg_enc_free(SSJpegEnc* j);

// ---- ss_gsi.hip
struct SSGsi;
int  ss_gsi_max_len_impl();
int  ss_gsi_check_impl(int n_tracks, const int* offsets, const int* frames, const double* vals, const double* len_scale, double alpha,
                       const double* out, const int* status, std::string& err);
int  ss_gsi_smooth_impl(SSGsi** pg, hipStream_t stream, int n_tracks, const int* offsets, const int* frames, const double* vals,
                        const double* len_scale, double alpha, double* out, int* status, std::string& err);
void ss_gsi_free(SSGsi* g);

// ---- ss_mot.hip
struct SSMot;
int  ss_mot_max_boxes_impl();
int  ss_mot_check_impl(int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id, const int* tr_id,
                       const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                       const int* hota_idx, const double* hota_s, const int* clear_idx, const double* clear_s, std::string& err);
int  ss_mot_eval_impl(SSMot** pm, hipStream_t stream, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id,
                      const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                      int* hota_idx, double* hota_s, int* clear_idx, double* clear_s, double* ga, std::string& err);
int  ss_mot_max_ids_impl();
int  ss_mot_identity_check_impl(int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id, const int* tr_id,
                                const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                                const int* idtp, const int* gt_to_tr, std::string& err);
int  ss_mot_identity_impl(SSMot** pm, hipStream_t stream, int n_pairs, const int* frame_off, const int* gt_off, const int* tr_off, const int* gt_id,
                          const int* tr_id, const double* gt_box, const double* tr_box, const int* n_gt_ids, const int* n_tr_ids, double thr,
                          int* idtp, int* gt_to_tr, int* pot, std::string& err);
void ss_mot_free(SSMot* m);

// ---- ss_ap.hip
struct SSAp;
int  ss_ap_max_gts_impl();
int  ss_ap_max_cell_dets_impl();
int  ss_ap_max_keep_impl();
int  ss_ap_max_dets_impl();
int  ss_ap_check_impl(int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_image, const int* cell_gt_off,
                      const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
                      int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
                      const int* max_dets, const double* precision, const double* recall, const int* det_rank, const int* rec_match,
                      const int* rec_ignored, std::string& err);
int  ss_ap_eval_impl(SSAp** pp, hipStream_t stream, int similarity, int n_classes, int n_cells, const int* class_cell_off, const int* cell_gt_off,
                     const int* cell_det_off, const double* gt_boxes, const int* gt_crowd, const double* det_boxes, const double* det_scores,
                     int n_thrs, const double* iou_thrs, int n_recs, const double* rec_thrs, int n_areas, const double* areas, int n_max_dets,
                     const int* max_dets, double* precision, double* recall, int* det_rank, int* rec_match, int* rec_ignored, std::string& err);
void ss_ap_free(SSAp* p);

// ---- ss_zone.hip
struct SSZone;
int  ss_zone_max_lines_impl();
int  ss_zone_max_zones_impl();
int  ss_zone_max_vertices_impl();
int  ss_zone_max_live_impl();
int  ss_zone_create_check_impl(const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy, const int* poly_off, int n_zones,
                               std::string& err);
int  ss_zone_create_impl(SSZone** pz, hipStream_t st, int S, const ss_zone_config* cfg, const int* lines, int n_lines, const int* poly_xy,
                         const int* poly_off, int n_zones, std::string& err);
int  ss_zone_reset_impl(SSZone* z, hipStream_t st, int stream, std::string& err);
int  ss_zone_update_check_impl(int n_frames, const float* d_rows, const int* d_nrows, std::string& err);
int  ss_zone_update_impl(SSZone* z, hipStream_t st, int n_frames, const float* d_rows, const int* d_nrows, uint32_t* d_events, uint32_t* d_inside,
                         int* d_dwell, int* d_line_totals, int* d_occupancy, int* d_heat_frames, int* d_heat_max, std::string& err);
int  ss_zone_pending_impl(SSZone* z, hipStream_t st, std::string& err);
int  ss_zone_get_totals_impl(SSZone* z, hipStream_t st, int stream, int* frames, int* line_class, int* line_totals, int* zone_entries, int* zone_exits,
                             long long* zone_dwell_sum, int* zone_longest, int* zone_peak, int* heat_max, std::string& err);
int  ss_zone_get_heat_impl(SSZone* z, hipStream_t st, int stream, int* grid, std::string& err);
void ss_zone_shape_impl(const SSZone* z, int* S, int* heat, int* gh, int* gw, int* h, int* w);
void ss_zone_heat_device_impl(const SSZone* z, int stream, void** d_heat, void** d_max);
int  ss_zone_set_colormap_impl(SSZone* z, const uint8_t* bgr, std::string& err);
int  ss_zone_blend_check_impl(const uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_heat,
                              long long heat_frame_stride, const int* d_max, int max_stride, int alpha, std::string& err);
int  ss_zone_blend_impl(SSZone* z, hipStream_t st, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride,
                        const int* d_heat, long long heat_frame_stride, const int* d_max, int max_stride, int alpha, std::string& err);
void ss_zone_free(SSZone* z);

// ---- ss_redact.hip
int  ss_redact_max_regions_impl();
int  ss_redact_max_vertices_impl();
int  ss_redact_max_radius_impl();
long long ss_redact_scratch_bytes_impl(int batch, int h, int w);
int  ss_redact_check_impl(const uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_regions,
                          const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, const void* d_scratch,
                          long long scratch_bytes, std::string& err);
int  ss_redact_impl(hipStream_t st, uint8_t* d_frames, int batch, long long frame_batch_stride, int h, int w, int row_stride, const int* d_regions,
                    const int* d_region_off, const int* d_verts, int effect, int strength, int fill_bgr, void* d_scratch, std::string& err);

// ---- ss_mtmc.hip
struct SSBank;
struct SSMtmc;
int  ss_bank_max_ids_impl();
int  ss_mtmc_max_tracklets_impl();
int  ss_bank_create_impl(SSBank** pb, hipStream_t st, int S, int max_ids, std::string& err);
int  ss_bank_reset_impl(SSBank* b, hipStream_t st, int stream, std::string& err);
int  ss_bank_update_check_impl(int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats, std::string& err);
int  ss_bank_update_impl(SSBank* b, hipStream_t st, int n_frames, const float* d_rows, const int* d_nrows, const float* d_feats, std::string& err);
int  ss_bank_pending_impl(SSBank* b, hipStream_t st, std::string& err);
int  ss_bank_get_impl(SSBank* b, hipStream_t st, int stream, int cap, int* n, int* ids, int* counts, int* first, int* last, int* cls, float* desc,
                      std::string& err);
void ss_bank_free(SSBank* b);
int  ss_mtmc_link_check_impl(int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr, int min_rows,
                             const int* global_id, const double* merges, const int* n_merges, std::string& err);
int  ss_mtmc_link_impl(SSMtmc** pg, hipStream_t st, int T, const float* desc, const int* cam, const int* first, const int* last, const int* n, double thr,
                       int min_rows, int* global_id, double* merges, int* n_merges, float* dist_out, std::string& err);
void ss_mtmc_free(SSMtmc* g);

// ---- ss_slice.hip
struct SSSlice;
int  ss_slice_max_tiles_impl();
int  ss_slice_max_candidates_impl();
int  ss_slice_config_check_impl(const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile, int n_extra,
                                int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y, std::string& err);
int  ss_slice_config_impl(SSSlice** ps, const int* h_tiles, int n_tiles, int frame_h, int frame_w, int canvas_h, int canvas_w, int rows_per_tile,
                          int n_extra, int n_kpt, float kpt_gain, float kpt_pad_x, float kpt_pad_y, std::string& err);
int  ss_slice_nms_geom_impl(const SSSlice* s, float* d_geom, int batch, std::string& err);
int  ss_slice_letterbox_check_impl(const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, const void* d_dst, int dst_flags,
                                   int pad_value, std::string& err);
int  ss_slice_letterbox_impl(SSSlice* s, hipStream_t st, const uint8_t* d_src, int batch, long long src_batch_stride, int row_stride, void* d_dst,
                             int dst_flags, int pad_value, std::string& err);
int  ss_slice_merge_check_impl(const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride, long long frame_stride,
                               int mode, int metric, float thr, int agnostic, int out_cap, const float* d_out, int out_row_stride,
                               long long out_frame_stride, const int* d_out_count, const int* d_out_src, long long src_frame_stride, std::string& err);
int  ss_slice_merge_impl(SSSlice* s, hipStream_t st, const float* d_rows, const int* d_counts, int batch, int row_stride, long long tile_stride,
                         long long frame_stride, int mode, int metric, float thr, int agnostic, int out_cap, float* d_out, int out_row_stride,
                         long long out_frame_stride, int* d_out_count, int* d_out_src, long long src_frame_stride, std::string& err);
void ss_slice_free(SSSlice* s);

// ---- ss_aflink.hip
struct SSAflink;
long long ss_aflink_weight_floats_impl();
int  ss_aflink_max_component_impl();
int  ss_aflink_chunk_option(int value);
int  ss_aflink_set_weights_check_impl(const float* blob, long long n, std::string& err);
int  ss_aflink_set_weights_impl(SSAflink** pg, hipStream_t stream, const float* blob, std::string& err);
int  ss_aflink_cost_check_impl(int n, const int* offsets, const double* feats, int t0, int t1, double thr_s, long long cap, const int* pair_i,
                               const int* pair_j, const double* cost, const long long* n_pairs, std::string& err);
int  ss_aflink_cost_impl(SSAflink** pg, hipStream_t stream, int n, const int* offsets, const double* feats, int t0, int t1, double thr_s, long long cap,
                         int* pair_i, int* pair_j, double* cost, float* inputs, long long* n_pairs, std::string& err);
int  ss_aflink_match_check_impl(int n, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost, double thr_p, const int* successor,
                                std::string& err);
int  ss_aflink_match_impl(SSAflink** pg, hipStream_t stream, int n, long long n_pairs, const int* pair_i, const int* pair_j, const double* cost,
                          double thr_p, int* successor, std::string& err);
void ss_aflink_free(SSAflink* g);
