/*
 * odam_samples.h -- C ABI of the association network's validation samples, cut from a scene table on the device.
 *
 * Restates, without its file reads, what the reference builds per sampled frame:
 *   src/datasets/scan_net_track.py:285-341  ScanNetTrack.get_by_sequence   (_preprocess_tracks :201-243, _preprocess :173-199)
 *   src/datasets/scan_net_track.py:34-97    ScanNetTrack.collater          (detections padded with -1 to 30 slots)
 * Everything discrete (which objects are tracks of a frame, which rows they keep, the order of the detections, the pairs and the
 * cap at 30) is decided on the host (odam_amd/assoc_samples.py: plan); this library holds the scene and does the arithmetic.
 * Conventions as in odam_assoc.h: plain pointers and sizes, int return codes (0 ok, 1 refused argument, 2 HIP error, 3 outside the
 * limits; odam_last_error() names the reason), the caller's stream, arguments refused before the device is touched.
 */
#ifndef ODAM_SAMPLES_H
#define ODAM_SAMPLES_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct odam_samples odam_samples;

/* A store for ONE scene of n_obj objects and n_frames frames with n_obs valid observations and n_unm unmatched detections in all
 * (n_unm may be 0).  Host bookkeeping only: no device call is made.  Code 3: n_obj, n_frames or n_obs below 1, n_unm below 0,
 * n_obs above n_obj * n_frames, or a count that does not fit 31 bits. */
int odam_samples_create(int n_obj, int n_frames, long long n_obs, long long n_unm, odam_samples** out);
int odam_samples_destroy(odam_samples* s);

/* Uploads the compacted scene (all arrays [host], float64 unless said otherwise) and makes every device allocation the store will
 * ever own; odam_samples_cut allocates nothing.  Returns after the copies have completed.
 *   obs      [n_obs, 78]           the valid rows of the table, object after object in frame order, column 14 (ground-truth id) removed
 *   obs_off  [n_obj + 1] int64     obs_off[o] .. obs_off[o + 1]: the rows of object o (at most n_frames of them)
 *   proj     [n_obj, n_frames, 4]  columns 79-82 of the table: the object's projected box in that frame, pixels
 *   cam      [n_frames, 13]        rows 0-2 of inv(T_wc) of the frame, row-major, and the camera azimuth
 *   unm      [n_unm, 78]           the unmatched detections, frame after frame, column 14 removed (may be null when n_unm == 0)
 *   unm_off  [n_frames + 1] int64
 * Code 1: a null pointer, offsets that do not start at 0, decrease, give an object more than n_frames rows or do not end at the
 * counts of odam_samples_create; an image size that is not positive. */
int odam_samples_load(odam_samples* s, const double* obs, const long long* obs_off, const double* proj, const double* cam,
                      const double* unm, const long long* unm_off, double img_w, double img_h, void* stream);

/* ONE launch for a batch of B samples.  All plan arrays [host] int32:
 *   frames [B]            the sampled frame of each sample
 *   n_det [B]             its detection count, after the cap
 *   det_src [B, 30]       source of detection j: r >= 0 row r of obs, r < 0 row -(r + 1) of unm (entries past n_det are not read)
 *   slot_sample [sum_t]   the sample of every track slot, not decreasing (the slots of a sample stand together, in track order)
 *   slot_obj [sum_t]      its object
 *   slot_row0 [sum_t]     its first kept row in obs
 *   slot_k [sum_t]        its row count, 1 .. n_times: rows slot_row0 .. slot_row0 + k lie inside the object's block
 * Outputs [dev]: tracks [sum_t, 79, n_times] float32 (channel-major, -1 past k), detections [B, 79, 30] float32 (-1 past n_det),
 * status [B] int32: bit 1 = a live track of the sample has a projected box of all -1 in the sampled frame (the reference's
 * assert "wrong projected bbox").  The layout is odam_assoc_forward_batch's when n_times = 100.
 * Per value: float64 arithmetic in a fixed order (t_co = ((x c0 + y c1) + z c2) + c3 with every product and sum rounded to nearest,
 * no contraction; box / size and the clip in float64; sin / cos in float64), rounded to float32 once.  A slot's output depends on
 * that slot's plan entries alone: the same bits wherever it stands in the batch.
 * Code 3: B outside 1..64, sum_t outside 1..1024, n_times outside 1..128, an n_det outside 1..30, a slot_k outside 1..n_times.
 * Code 1: a null pointer, a frame outside the scene, a slot or a detection source outside the store, slot_sample out of order,
 * a store that was not loaded. */
int odam_samples_cut(odam_samples* s, int B, const int* frames, const int* n_det, const int* det_src, int sum_t,
                     const int* slot_sample, const int* slot_obj, const int* slot_row0, const int* slot_k, int n_times,
                     float* tracks, float* detections, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
