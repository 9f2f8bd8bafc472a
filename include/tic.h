/*
 * tic.h — C-ABI of libtic.so, the MI355X (gfx950) encode/decode hot path of the
 * learned image codec in bolin-chen/tf_image_compression.
 *
 * The reference has no FFI: its hot path is a TF-1.x graph built by
 * model_N.encoder/decoder and run by tf.Session.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference root).  All
 * arguments are plain pointers and sizes; tensors are C-contiguous NHWC.  Every
 * function returns 0 on success or a negative TIC_E* code; tic_last_error()
 * returns a thread-local message for the last failure on the calling thread.
 *
 * Host pointers (tic_encode / tic_decode / tic_rmbe) are owned by the caller and are
 * only read/written during the call.  Device pointers (the *_device variants) must
 * come from tic_device_alloc on the same handle; those calls are asynchronous on the
 * handle's HIP stream — use tic_synchronize() before reading results.
 */
#ifndef TIC_H_
#define TIC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIC_OK 0
#define TIC_EINVAL (-1)     /* bad argument / shape (reference: ValueError, tf.errors.InvalidArgumentError) */
#define TIC_ENOTFOUND (-2)  /* unknown variable name (reference: Saver.restore NotFoundError) */
#define TIC_ESTATE (-3)     /* handle not finalized / missing weights */
#define TIC_EHIP (-4)       /* HIP runtime error */
#define TIC_ENOMEM (-5)
#define TIC_EUNSUPPORTED (-6)
#define TIC_EOVERFLOW (-7)  /* value does not fit (reference: OverflowError) */
#define TIC_EIO (-8)        /* file I/O (reference: IOError / RuntimeError) */

#define TIC_MODEL_RMBE 100  /* submit/2/rmbe/model.py:113 (block-effect post-filter) */
#define TIC_MODEL_CH128 128 /* base_model/ch_128/model.py:34-215 (128-channel trunk, P/4 code) */

typedef struct tic_handle tic_handle;

/* Library / build identification. */
const char* tic_version(void);
const char* tic_last_error(void);

/* Open a codec for model_N on HIP device `device`.
 * Replaces: `from model_N import model` (encode.py:225-232, decode.py:280-287,
 *   submit/encoder.py:220-223) + model_N/config.json's patch_size/quan_scale
 *   (encode.py:129-145) + os.environ['CUDA_VISIBLE_DEVICES']=gpu (encode.py:218).
 * model_id: 0..3, TIC_MODEL_CH128 or TIC_MODEL_RMBE.  patch_size: even, >= 16 (for rmbe: 128).
 * quan_scale: Q in [2, 256] (model_0/config.json:6). */
int tic_create(int model_id, int patch_size, int quan_scale, int device, tic_handle** out);
void tic_destroy(tic_handle* h);

/* Channel statistics (float32 [3]).
 * Replaces: np.load('data_info/channel_normalization_params.npz') at model import
 *   (model_0/model.py:18,26-28; submit/2/rmbe/model.py:25-30). */
int tic_set_normalization(tic_handle* h, const float* mean3, const float* std3);

/* One TF variable, by its scope name and TF layout: '<scope>/kernel' HWIO [3,3,Cin,Cout]
 * for conv (basic_block/basic_block.py:30), [3,3,Cout,Cin] for conv-transpose (:53);
 * '<scope>/bias' [Cout] (:35,:59).  Copied and repacked at tic_finalize.
 * Replaces: tf.train.Saver().restore (utils/utils.py:84-93), one variable at a time. */
int tic_set_param(tic_handle* h, const char* name, const float* data, const int64_t* shape, int ndim);

/* Check every variable is present, repack and upload.  (Saver.restore's all-or-nothing.) */
int tic_finalize(tic_handle* h);

/* Shape of the quantised code for one patch (h, w, C).
 * Replaces: encoded_patches[0][0].shape (encode.py:171) / get_encoded_shape (decode.py:130-140). */
int tic_code_shape(const tic_handle* h, int* eh, int* ew, int* ec);

/* Encoder: uint8 RGB patches [n,P,P,3] -> uint8 symbols [n,eh,ew,ec] in {0..Q-1}
 * (optional float32 pre-quantiser activations [n,eh,ew,ec] for parity checks).
 * Replaces: model.encoder(input, patch_size, quan_scale) (model_0/model.py:34-144)
 *   + the sess.run loop (encode.py:157-165) + astype(int) (encode.py:182). */
int tic_encode(tic_handle* h, const uint8_t* patches, int n, uint8_t* idx_out, float* preact_out);

/* Decoder: uint8 symbols [n,eh,ew,ec] -> uint8 RGB [n,P,P,3] (np.around half-even of the
 * clipped float) and/or the float32 reconstruction in [0,255] (either may be NULL).
 * Replaces: model.decoder(input, quan_scale) (model_0/model.py:147-263) + sess.run loop
 *   (decode.py:212-220) + np.around(...).astype(np.uint8) (decode.py:249). */
int tic_decode(tic_handle* h, const uint8_t* idx, int n, uint8_t* rgb_out, float* f32_out);

/* Block-effect post-filter network on float32 RGB windows [n,128,128,3] -> float32 (clipped).
 * Handle must be created with TIC_MODEL_RMBE.
 * Replaces: rmbe_model.model(patch_batch) + sess.run (submit/2/rmbe/model.py:113-197,
 *   submit/2/rmbe/rmbe.py:28-67). */
int tic_rmbe(tic_handle* h, const float* windows, int n, float* out);

/* --- device-resident variants (benchmarks, multi-stage pipelines) --- */
int tic_device_alloc(tic_handle* h, size_t bytes, void** dptr);
int tic_device_free(tic_handle* h, void* dptr);
int tic_memcpy_h2d(tic_handle* h, void* dst, const void* src, size_t bytes);
int tic_memcpy_d2h(tic_handle* h, void* dst, const void* src, size_t bytes);
int tic_synchronize(tic_handle* h);
int tic_encode_device(tic_handle* h, const uint8_t* d_patches, int n, uint8_t* d_idx, float* d_preact);
int tic_decode_device(tic_handle* h, const uint8_t* d_idx, int n, uint8_t* d_rgb, float* d_f32);
/* encode then decode back-to-back on the handle's stream (the benchmark step). */
int tic_codec_device(tic_handle* h, const uint8_t* d_patches, int n, uint8_t* d_idx, uint8_t* d_rgb);
int tic_rmbe_device(tic_handle* h, const float* d_windows, int n, float* d_out);

/* Options: "streams" (1 or 2 execution lanes; with 2, every batch chunk is split in halves
 * on two HIP streams that run concurrently — default 2, env TIC_STREAMS), "chunk" (max
 * patches per launch sequence, default 256, env TIC_MAX_CHUNK), "graph" (1: replay
 * tic_codec_device as a captured HIP graph per (buffers, n) — default 0: measured slower
 * than eager dual-lane launches on MI355X), "persist_grid" (> 0: cap on the grid of the
 * persistent conv variants, so that tests run several tiles per workgroup; default 0),
 * "poison" (test hook, default 0; 1: every pass of the layer runner — behind tic_encode[_device],
 * tic_decode[_device], tic_codec_device, tic_rmbe[_device] and tic_rmbe_image_device — first fills,
 * on its lane's own stream, the lane's three activation workspaces, the lane's chain hand-off
 * buffer and the slices of the handle's own output staging (host entries, whole-image windows) it
 * is about to write with the 32-bit word 0x7FC5A5A5: a NaN as float, the bytes 165, 165, 197, 127
 * as symbols or pixels.  A kernel that leaves an element unwritten, or reads a hand-off before it
 * is published, then no longer finds the previous run's value there.  The hand-off flags and
 * control words, timing-probe buffers, weights, tables, input staging and every caller-owned
 * buffer are left alone; tic_autotune, tic_autotune_step and tic_profile_layers run without the
 * fills.  "poison" 1 and "graph" 1 exclude each other: whichever is set second is TIC_EINVAL).
 * Structural, bit-identical fusions (1 on, 0 off, -1 the model's default): "fuse01"
 * (encode_0 + encode_1 in one launch; default on), "fuse_tail" (decode_1 + decode_0; on),
 * "chain" (each run of stride-1 64->64 layers in one launch; on for models 0-2, off for
 * model_3 / rmbe; declined automatically where the geometry cannot run it), "chain_wh"
 * (1 or 2), "chain_x" (1: the encoder's stride-2 layer in front of a run and the decoder's
 * transposed layer behind it run inside the chain's launch; 2: also the decoder's next
 * transposed layer (decode_2); needs chain_wh 2; default 1 for models 0-2, the shipped tuning
 * decides), "chain_j" (tic_codec_device only: the encoder's last chain launch — head, run,
 * quantiser — and the decoder's first — dequantiser, run, tail — as one launch, where both are
 * planned on the same stage with chain_x; tic_encode_device / tic_decode_device keep their
 * launches; default 1 for models 0-2, env TIC_CHAIN_J), "chain_order" (region placement: 0 atomic ticket, 1 blockIdx, 2 a
 * patch's regions on one XCD, -1 automatic), "s1_form" (stride-1 form: 0 direct, 1 Winograd F(2x2,3x3), 2 Winograd F(4x4,3x3)
 * for the 64->64 res-block convs, other layers falling back to 1; -1 the model's default: 2 for
 * model_3 and the rmbe net, 1 otherwise; env TIC_S1_FORM=direct|wino|wino4), "s2_form" (standalone
 * stride-2 / transposed layers: 0 direct, 1 polyphase Winograd — layers a fused kernel could run
 * keep the direct form; -1 the model's default: 1 for models 0, 1 and 3 (80-channel layers direct), 0 otherwise; env TIC_S2_FORM=direct|pwino), "decouple" (lanes fork from the
 * handle stream only when a call's device byte ranges or earlier non-lane work require it;
 * default 1), "mark_layer" (see tic_mark_durations). */
int tic_set_option(tic_handle* h, const char* key, int value);

/* --- introspection / measurement --- */
int tic_num_layers(const tic_handle* h);
/* kind: 0 conv s1, 1 conv s2, 2 conv-transpose s2; act: 0 identity, 1 relu;
 * stage: 0 encoder, 1 decoder.  name_buf receives the TF scope (NUL-terminated). */
int tic_layer_info(const tic_handle* h, int i, char* name_buf, int name_len, int* kind, int* cin,
                   int* cout, int* act, int* stage, int* residual);
/* Static layer table keyed by model id (no handle, no device needed). */
int tic_model_num_layers(int model_id);
int tic_model_layer(int model_id, int i, char* name_buf, int name_len, int* kind, int* cin, int* cout,
                    int* act, int* stage, int* residual);
/* Time each layer's kernel with HIP events on the handle's stream over `iters` runs of
 * tic_codec_device(n) (or the rmbe net); writes the mean ms per launch of layer i to
 * ms_out[i] (size >= tic_num_layers). */
int tic_profile_layers(tic_handle* h, const void* d_in, int n, int iters, float* ms_out);
/* In-step launch timing (bench.py's roofline): with option "mark_layer" = i (>= 0) every
 * lane records a HIP event pair on its own stream around each launch that starts at layer i
 * (a fused or chained launch starts at its first layer) during ordinary tic_codec_device /
 * encode / decode calls, up to 1024 pairs per lane.  tic_mark_durations synchronises,
 * writes up to cap durations (ms) to ms_out, returns how many, and clears the record. */
int tic_mark_durations(tic_handle* h, float* ms_out, int cap);

/* Measure every compiled tiling of every layer on the live buffers of one encode+decode
 * (or rmbe) pass over d_in[n] and keep the fastest per layer for batch size n (like
 * cuDNN's benchmark mode).  Untuned batch sizes use a grid-size heuristic. */
int tic_autotune(tic_handle* h, const void* d_in, int n, int reps);
/* In-situ tuning for tic_codec_device / tic_rmbe_device on n patches: each layer's
 * variant is chosen by the time of the whole launch sequence as it runs (both lanes),
 * greedy over the layers for `rounds` passes, each candidate timed as `reps` steps (min
 * of 3).  Starts from tic_autotune's per-layer choice (run here if missing).  All
 * candidates produce bit-identical results. */
int tic_autotune_step(tic_handle* h, const void* d_in, int n, int rounds, int reps);
/* Tiling used by layer i for batch n: rows per workgroup and channel split, the latter
 * + 100 when the weights are staged through LDS (0,0 if the layer has one fixed kernel). */
int tic_layer_variant(const tic_handle* h, int i, int n, int* th, int* nsplit);
/* Kernel instance layer i launches for batch n, as "<kernel>" "<template args>" in the
 * form tools/pmc_summary.py prints (e.g. "conv3x3<1,32,32,4,4,1,false,1,false,0,0>");
 * empty when the layer runs inside the previous layer's launch.  cap includes the NUL. */
int tic_layer_kernel(const tic_handle* h, int i, int n, char* name, int cap);
/* The same for the launches of tic_codec_device.  They are tic_layer_kernel's except where
 * option "chain_j" joins the encoder's last and the decoder's first chain launch: the joined
 * launch is named at its first layer (HT bit 16 set) and every other layer of it is empty. */
int tic_codec_kernel(const tic_handle* h, int i, int n, char* name, int cap);
/* Tuning state as text (every tuned tiling / variant per layer and batch key, and the
 * structural fusion flags), so a tuning run can be replayed exactly by another process of
 * the same build (like cuDNN's find-db): returns the length (excluding the NUL) and writes
 * it when cap is large enough.  tic_tuning_import validates every entry against the
 * layer table and the compiled registries (TIC_EINVAL on any mismatch, nothing applied). */
int tic_tuning_export(const tic_handle* h, char* buf, int cap);
int tic_tuning_import(tic_handle* h, const char* text);

/* Unit-test entry: one layer on device float32 NHWC tensors.
 * kind/act as tic_layer_info; res (nullable) is added after the activation.
 * w is the TF-layout kernel (HWIO for conv, [3,3,Cout,Cin] for conv-T), host memory.
 * in: [n,H,W,cin]; out: [n,Ho,Wo,cout]. */
int tic_conv3x3_device(tic_handle* h, int kind, int act, const float* d_in, int n, int H, int W, int cin,
                       int cout, const float* w_host, const float* b_host, const float* d_res, float* d_out);

/* The handle's HIP stream (hipStream_t as void*), e.g. to enqueue an RCCL collective
 * behind the codec's kernels.  Work enqueued there is ordered before every later codec
 * call: from this call on the handle's execution lanes fork from the stream at every call
 * (see tic_stream_external). */
int tic_get_stream(tic_handle* h, void** stream);
/* Declare whether the caller may have work of its own pending on the handle's stream
 * (1, the state after tic_get_stream) or synchronises everything it enqueues there before
 * the next codec call (0): then the lanes fork from the stream only after the handle's own
 * copies / glue kernels, and each lane starts its next batch as soon as it is free. */
int tic_stream_external(tic_handle* h, int on);

/* Device info string (name, CUs, arch) for logs. */
int tic_device_info(tic_handle* h, char* buf, int len);

/* --- whole images (BASELINE config 5) and symbol statistics; device pointers, async on
 * the handle's stream.  Any handle may run the glue kernels; tic_rmbe_image_device needs
 * a TIC_MODEL_RMBE handle. --- */

/* Reflect-pad an HWC uint8 image [H,W,3] bottom/right to multiples of P (np.pad 'reflect':
 * edge pixel not repeated, any pad length) and cut row-major PxP patches into
 * d_patches [ceil(H/P)*ceil(W/P), P, P, 3] (4-byte aligned; P a multiple of 4).
 * Replaces: utils.crop_image_input_patches (utils/utils.py:96-133), encode.py:154-156. */
int tic_image_to_patches_device(tic_handle* h, const uint8_t* d_img, int H, int W, int P, uint8_t* d_patches);

/* Stitch row-major float32 patches [ceil(H/P)*ceil(W/P), P, P, 3] into an HWC image cropped
 * to HxW.  Replaces: utils.concat_patches (utils/utils.py:136-167), decode.py:222-230. */
int tic_patches_to_image_device(tic_handle* h, const float* d_patches, int H, int W, int P, float* d_img);

/* Block-effect post-filter of a whole float32 HWC image [H,W,3] in [0,255], in place: the
 * 128x128 windows at column offset 64 (all full rows of windows), filtered and written back,
 * then the windows at row offset 64; edge strips that fill no window stay untouched.
 * Replaces: rmbe.rmbe / rmbe_height / rmbe_width (submit/2/rmbe/rmbe.py:15-111) with the
 * network of submit/2/rmbe/model.py:113-197 (one handle, no per-call graph rebuild). */
int tic_rmbe_image_device(tic_handle* h, float* d_img, int H, int W);

/* --- lists of different-sized images as ONE patch batch.  The reference handles images one
 * after another (encode.py:152 "To be paralleled"); patches are independent, so the images of
 * a list share one launch sequence.  Image i lies in a device arena at offsets[i], counted in
 * elements of the arena's type (bytes of the uint8 arena, floats of the float32 arena — the
 * same array serves both); offsets may have any alignment, any order and gaps.  offsets /
 * heights / widths are HOST arrays of n_images entries (heights, widths > 0, offsets >= 0),
 * read during the call only.  Asynchronous on the handle's stream, no host synchronisation.
 * n_images == 0 does nothing.  tic_encode_device / tic_decode_device / tic_round_u8_device
 * run on the patch batch / the arena unchanged. --- */

/* tic_image_to_patches_device of every image in one launch: d_patches
 * [sum_i ceil(H_i/P)*ceil(W_i/P), P, P, 3], the patches of image i behind those of image
 * i-1, row-major within an image; *n_patches_out receives the sum. */
int tic_images_to_patches_device(tic_handle* h, const uint8_t* d_images, const int64_t* offsets,
                                 const int32_t* heights, const int32_t* widths, int n_images, int P,
                                 uint8_t* d_patches, int* n_patches_out);

/* tic_patches_to_image_device of every image in one launch (the inverse layout, float32,
 * each image cropped to H_i x W_i).  Arena elements that belong to no image are not written;
 * TIC_EINVAL when the ranges of two images overlap. */
int tic_patches_to_images_device(tic_handle* h, const float* d_patches, const int64_t* offsets,
                                 const int32_t* heights, const int32_t* widths, int n_images, int P,
                                 float* d_images);

/* tic_rmbe_image_device of every image of a float32 arena, in place: the column-offset windows
 * of ALL images in one gather, one run of the network and one write-back, then the row-offset
 * windows likewise (exact: pass 2 of an image depends only on pass 1 of the same image).
 * TIC_MODEL_RMBE handle; TIC_EINVAL when the ranges of two images overlap. */
int tic_rmbe_images_device(tic_handle* h, float* d_images, const int64_t* offsets, const int32_t* heights,
                           const int32_t* widths, int n_images);

/* np.around(x).astype(np.uint8) of n float32 values in [0,255] (half to even; clamped).
 * Replaces: submit/2/decoder.py:176, decode.py:249. */
int tic_round_u8_device(tic_handle* h, const float* d_in, size_t n, uint8_t* d_out);

/* Accumulate np.histogram(symbols, bins=range(Q+1))[0] of n uint8 symbols into the uint64
 * counts d_counts[Q] (d_sym 4-byte aligned, d_counts 8-byte aligned; zero it first with
 * tic_memset_device).  Replaces: get_encoded_distribution.py:113-126 (the per-batch
 * histogram of the encoder output summed over the data set). */
int tic_histogram_device(tic_handle* h, const uint8_t* d_sym, size_t n, int Q, uint64_t* d_counts);

/* Accumulate the exact sum of squared differences of two uint8 arrays of n bytes into
 * *d_acc (uint64; 4-byte aligned inputs).  Replaces: evaluate.mse summed over a data set
 * (processing_utils/evaluate.py:10-32; dataset PSNR = 10 log10(255^2 sum(dims)/sum(SSE))). */
int tic_sse_u8_device(tic_handle* h, const uint8_t* d_a, const uint8_t* d_b, size_t n, uint64_t* d_acc);

/* --- MS-SSIM (Wang et al. 2003 with the choices of tf.image.ssim_multiscale: 11-tap Gaussian
 * window of sigma 1.5, "valid" filtering, C1 = (0.01*255)^2, C2 = (0.03*255)^2, five scales, each
 * the 2x2 mean of the one before with an odd last row / column paired with itself) of lists of
 * uint8 HWC image pairs.  Replaces: nothing in the reference's own code — processing_utils/
 * evaluate.py:10-32 has the PSNR only, while the CLIC challenge the codec was built for
 * (submit/) ranks by PSNR and MS-SSIM, computed by the organisers' host script. --- */

/* Bytes of device scratch tic_msssim_images_device needs for images of these sizes (pyramid
 * planes and per-workgroup partial sums).  Host arithmetic: no device, no handle.  TIC_EINVAL
 * for a null pointer, a negative count or a side below 161 (161 -> 81 -> 41 -> 21 -> 11). */
int tic_msssim_scratch_bytes(const int32_t* heights, const int32_t* widths, int n_images, size_t* bytes);

/* Image i of both uint8 arenas lies at byte offsets[i] (any alignment, order, gaps; HOST arrays
 * as for the image-list entries above).  d_out: double [n_images][5][3][2], fully overwritten:
 * [j][c][0] = sum of cs, [j][c][1] = sum of l*cs over the (h_j-10)(w_j-10) valid positions of
 * scale j and channel c (per-position values float32, sums float64); the host forms
 * prod_j max(mean cs_j, 0)^w_j * max(mean ssim_4, 0)^w_4 per channel and averages the channels.
 * Asynchronous on the handle's stream, no host synchronisation, any list length; d_scratch
 * (8-byte aligned, caller-owned) is only used during the call's kernels.  Deterministic (no
 * floating-point atomics): the 30 doubles of an image are bit-identical from call to call and do
 * not depend on the other images, on its position in the list or on its offset.  TIC_EINVAL with
 * nothing launched for a null handle / pointer, a side below 161, a negative count or a scratch
 * that is too small; n_images == 0 does nothing. */
int tic_msssim_images_device(tic_handle* h, const uint8_t* d_a, const uint8_t* d_b, const int64_t* offsets,
                             const int32_t* heights, const int32_t* widths, int n_images, void* d_scratch,
                             size_t scratch_bytes, double* d_out);

/* hipMemsetAsync on the handle's stream. */
int tic_memset_device(tic_handle* h, void* d_ptr, int value, size_t bytes);

/* Make `waiter`'s stream wait for all work enqueued so far on `signaler`'s stream (same
 * device): chains a codec handle and an rmbe handle without a host synchronisation. */
int tic_stream_wait(tic_handle* waiter, tic_handle* signaler);
/* Named dependencies (slot 0..7): tic_event_record marks the point reached so far on h's
 * stream; tic_stream_wait_event makes `waiter`'s stream wait for the last mark of that
 * slot on `signaler` (no-op if never recorded).  Lets a pipeline wait for exactly the
 * work that last used a buffer (e.g. the rmbe pass of image i-2 before the codec of
 * image i reuses its stitch buffer) instead of everything enqueued so far. */
int tic_event_record(tic_handle* h, int slot);
int tic_stream_wait_event(tic_handle* waiter, tic_handle* signaler, int slot);

/* CRC-32C (Castagnoli) of n bytes, continuing `crc` (0 to start).  Host only.  Used by the
 * TensorFlow checkpoint reader that replaces tf.train.Saver.restore (utils/utils.py:84-93):
 * table blocks and tensor-bundle entries carry masked CRC-32C checksums. */
uint32_t tic_crc32c(const void* data, size_t n, uint32_t crc);

/* --- entropy coder (host, no device) ---
 * Replaces the third-party `range_coder` package used by encode.py:86-97 and
 * decode.py:89-99: RangeEncoder(path).encode(data, cum_freq) / .close() and
 * RangeDecoder(path).decode(n, cum_freq) / .close().  cum_freq: non-decreasing int64
 * table starting at 0, entries < 2^32 (else TIC_EOVERFLOW), total <= 2^24.  Symbols
 * with zero frequency or outside the table are TIC_EINVAL; calls after close are
 * TIC_ESTATE.  Several encode() calls append to one stream. */
typedef struct tic_rc_encoder tic_rc_encoder;
typedef struct tic_rc_decoder tic_rc_decoder;
const char* tic_rc_last_error(void);
int tic_rc_encoder_open(const char* path, tic_rc_encoder** out);
int tic_rc_encode(tic_rc_encoder* e, const int64_t* data, size_t n, const int64_t* cum_freq, size_t ncum);
int tic_rc_encoder_close(tic_rc_encoder* e);
void tic_rc_encoder_free(tic_rc_encoder* e);
int tic_rc_decoder_open(const char* path, tic_rc_decoder** out);
int tic_rc_decode(tic_rc_decoder* d, size_t n, const int64_t* cum_freq, size_t ncum, int64_t* out);
int tic_rc_decoder_close(tic_rc_decoder* d);
void tic_rc_decoder_free(tic_rc_decoder* d);

/* --- segmented range-coder stream, version 1 (host part: no device) ---
 * One container per symbol sequence, all integers little-endian:
 *   0  4   magic "TICS"          8  4  L: symbols per segment (multiple of 4, 4..16384)
 *   4  1   version = 1           12 8  n: symbols in the stream (> 0)
 *   5  3   zero                  20 2*S u16 payload length of each segment, S = ceil(n / L)
 *   then the S payloads back to back.
 * Segment j holds symbols [j*L, min((j+1)*L, n)); its payload is exactly what
 * tic_rc_encoder_open / tic_rc_encode / tic_rc_encoder_close write for those symbols (the minimal
 * flush included; at most 3*len + 4 bytes) and decodes like that file (zeros past its end).
 * Segments are independent streams, so the device entries below code one per lane.  Symbols are
 * bytes: cum_freq as above with at most 257 entries and every frequency > 0.  Errors leave
 * their message in tic_rc_last_error. */

/* Worst-case container size: 20 + 2*S + 3*n + 4*S.  TIC_EINVAL for a bad L or n == 0. */
int tic_rcseg_bound(size_t n, uint32_t L, size_t* bytes);
/* Writes the container of sym[0..n) into out[0..cap) and its size into *written.  TIC_EINVAL for
 * cap < tic_rcseg_bound, a bad table or a symbol outside it. */
int tic_rcseg_encode(const uint8_t* sym, size_t n, uint32_t L, const int64_t* cum_freq, size_t ncum, uint8_t* out,
                     size_t cap, size_t* written);
/* Full validation: magic, version, reserved bytes, L, n > 0, the whole length table present,
 * every length <= 3*len_j + 4, lengths summing to exactly the bytes that remain.  L / n may be
 * NULL.  TIC_EINVAL otherwise. */
int tic_rcseg_parse(const uint8_t* buf, size_t nbytes, uint32_t* L, uint64_t* n);
/* tic_rcseg_parse, then TIC_EINVAL when n differs from the header's, then the n symbols. */
int tic_rcseg_decode(const uint8_t* buf, size_t nbytes, const int64_t* cum_freq, size_t ncum, uint8_t* sym_out,
                     size_t n);

/* --- segmented range-coder stream, version 2: a periodic context model (host part) ---
 * The stream is coded under K cumulative tables; symbol k of the stream uses table k mod K (K = the
 * code's channel count: one table per channel; K = the symbols of a patch: one per code
 * position; K = 1: the model of version 1).  The container is version 1 with a 28-byte header:
 *   0..19  as version 1, version byte = 2
 *   20 4   K                      24 4  CRC-32C (tic_crc32c) of the K*ncum table entries as int64,
 *   28     the u16 length table, then the payloads        little-endian, row-major
 * Segment j starts at context (j*L) mod K (K need not divide L); its payload is what
 * tic_rc_encode writes when every symbol is passed in a call of its own with its context's table.
 * tables: K rows of one common ncum (2..257), each row a table as version 1 asks for; rows may
 * have different totals.  1 <= K <= 65536 and K*ncum <= 262144. */

/* tic_rcseg_bound + 8. */
int tic_rcseg_bound_ctx(size_t n, uint32_t L, size_t* bytes);
/* As tic_rcseg_encode, under tables[K][ncum]. */
int tic_rcseg_encode_ctx(const uint8_t* sym, size_t n, uint32_t L, const int64_t* tables, size_t K, size_t ncum,
                         uint8_t* out, size_t cap, size_t* written);
/* tic_rcseg_parse's validation of a version-2 container (a version-1 container is TIC_EINVAL, as
 * a version-2 one is for tic_rcseg_parse); also the header's K and CRC.  Outputs may be NULL. */
int tic_rcseg_parse_ctx(const uint8_t* buf, size_t nbytes, uint32_t* L, uint64_t* n, uint32_t* K, uint32_t* crc);
/* tic_rcseg_parse_ctx, TIC_EINVAL when n, K or the CRC of `tables` differ from the header's, then
 * the n symbols. */
int tic_rcseg_decode_ctx(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K, size_t ncum,
                         uint8_t* sym_out, size_t n);

/* --- segmented range-coder stream, version 3: causal-neighbour contexts (host part) ---
 * The stream is coded under K = K0*M cumulative tables of one common ncum; nsym = ncum - 1.  The
 * container carries the code geometry (eh, ew, C), neighbours in {1, 2} (1: W; 2: W and N) and
 * M = 3^neighbours.  For symbol k of the stream (patch-major, then h, w, C):
 *   p = k mod (eh*ew*C), h = p div (ew*C), w = (p div C) mod ew, seg0 = L*floor(k / L)
 *   W neighbour jW = k - C,    valid iff w >= 1 and jW >= seg0
 *   N neighbour jN = k - ew*C, valid iff h >= 1 and jN >= seg0
 *   t(j) = 0 when j is invalid, else 1 + class(sym[j]); class(s) = 1 if 2*s >= nsym, else 0
 *   nb = t(jW) (neighbours = 1), t(jW) + 3*t(jN) (neighbours = 2)
 * and symbol k is coded under table row (k mod K0)*M + nb.  K0 = C gives channel x neighbours
 * (the intended use); K0 = 1 and K0 = eh*ew*C are legal.  A neighbour outside the symbol's own
 * segment never counts, so segments stay independent streams; n need not be a multiple of the
 * patch size and L need not relate to the geometry.  The container is version 2's with a 36-byte
 * header:
 *   0..19  as versions 1 and 2, version byte = 3
 *   20 4   K0                     24 4  CRC-32C (tic_crc32c) of the K*ncum table entries as int64,
 *   28 6   u16 eh, u16 ew, u16 C        little-endian, row-major
 *   34 1   neighbours             35 1  zero
 *   36     the u16 length table, then the payloads
 * A segment's payload is what tic_rc_encode writes when every symbol is passed in a call of its
 * own under the row above.  tables: K rows, each validated as version 2 validates its rows (rows
 * the geometry never reaches included).  1 <= eh, ew, C <= 65535, K0 >= 1, K*ncum <= 262144. */

/* tic_rcseg_bound + 16. */
int tic_rcseg_bound_nbr(size_t n, uint32_t L, size_t* bytes);
/* As tic_rcseg_encode, under tables[K0][M][ncum]. */
int tic_rcseg_encode_nbr(const uint8_t* sym, size_t n, uint32_t L, const int64_t* tables, size_t K0,
                         uint32_t neighbours, size_t ncum, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* out,
                         size_t cap, size_t* written);
/* tic_rcseg_parse's validation of a version-3 container (versions 1 and 2 are TIC_EINVAL, as
 * version 3 is for tic_rcseg_parse and tic_rcseg_parse_ctx), the reserved byte, neighbours in
 * {1, 2}, the geometry and K0 within their limits.  Outputs may be NULL. */
int tic_rcseg_parse_nbr(const uint8_t* buf, size_t nbytes, uint32_t* L, uint64_t* n, uint32_t* K0, uint32_t* crc,
                        uint32_t* eh, uint32_t* ew, uint32_t* C, uint32_t* neighbours);
/* tic_rcseg_parse_nbr, TIC_EINVAL when n, K0, the geometry, neighbours or the CRC of `tables`
 * differ from the header's, then the n symbols. */
int tic_rcseg_decode_nbr(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K0, uint32_t neighbours,
                         size_t ncum, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* sym_out, size_t n);

/* --- symbol ranges of a segmented stream (host part) ---
 * Symbol k of a stream lies in segment k / L, and segments are independent streams, so symbols
 * [first, first + count) need segments j0 = first / L .. j1 = (first + count - 1) / L and nothing
 * else.  Version 2's context phase and version 3's position, K0 phase and neighbour validity all
 * follow from the absolute index k, so the formats above are unchanged. */

/* The segment span (*j0, *nj = j1 - j0 + 1) of a symbol range and the byte extent [*byte_off,
 * *byte_off + *byte_len), relative to the container's start, of those segments' payloads.  Works
 * on a container of any of the three versions, following its version byte, and needs only the
 * header and the u16 length table in buf[0..nbytes): payload bytes may be absent.  Outputs may be
 * NULL.  TIC_EINVAL for a bad header (magic, version, reserved bytes, L, n), a length table that
 * is not wholly present, count == 0 or a range that is not inside [0, n). */
int tic_rcseg_range_extent(const uint8_t* buf, size_t nbytes, size_t first, size_t count, size_t* j0, size_t* nj,
                           size_t* byte_off, size_t* byte_len);
/* tic_rcseg_decode / _ctx / _nbr of a symbol range: the same arguments and the same validation
 * (the whole container is parsed; n, K, K0, geometry, neighbours, CRC), then TIC_EINVAL for
 * count == 0 or a range not inside [0, n).  Write exactly count symbols to sym_out, equal to
 * sym[first .. first + count) of the full decode.  A segment is decoded from its start up to the
 * range's end; no payload byte outside tic_rcseg_range_extent's extent is read.  The full
 * decoders are these with the range [0, n).  They are the reference of the device entries
 * tic_entropy_decode_ranges*_device. */
int tic_rcseg_decode_range(const uint8_t* buf, size_t nbytes, const int64_t* cum_freq, size_t ncum, uint8_t* sym_out,
                           size_t n, size_t first, size_t count);
int tic_rcseg_decode_range_ctx(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K, size_t ncum,
                               uint8_t* sym_out, size_t n, size_t first, size_t count);
int tic_rcseg_decode_range_nbr(const uint8_t* buf, size_t nbytes, const int64_t* tables, size_t K0,
                               uint32_t neighbours, size_t ncum, uint32_t eh, uint32_t ew, uint32_t C,
                               uint8_t* sym_out, size_t n, size_t first, size_t count);

/* --- "TICA" version 1: a segmented stream that carries its own tables (host part) ---
 * Version 3's context model under tables fitted to the stream itself (semi-static two-pass
 * coding), so a decoder needs nothing but the container.  All integers little-endian:
 *    0 4  magic "TICA"               20 4  K0 (>= 1)
 *    4 1  version = 1                24 6  u16 eh, u16 ew, u16 C (each 1..65535)
 *    5 1  neighbours in {0, 1, 2}    30 2  zero
 *    6 2  nsym (2..256)              32 4  T = K0*M*(nsym-1)*2, the bytes of the table block
 *    8 4  L (multiple of 4, 4..16384) 36 4 CRC-32C (tic_crc32c) of the T table-block bytes
 *   12 8  n (> 0)                    40 T  table block
 *   40+T  the u16 payload length of each of the S = ceil(n/L) segments, then the S payloads
 * M = 3^neighbours.  The row of symbol k is version 3's (k mod K0)*M + nb, nb derived as above
 * (neighbours only inside the symbol's own segment, class(s) = 2*s >= nsym) and 0 when
 * neighbours = 0.  K0*M*(nsym+1) <= 262144.
 * Table block: rows r = 0 .. K0*M - 1, each nsym - 1 u16 frequencies f_0 .. f_{nsym-2}; the last
 * frequency is 4096 minus their sum.  Every frequency, the implied one included, is >= 1 and every
 * row's total is 4096.
 * Payloads: as versions 2 and 3, what tic_rc_encode writes with one call per symbol under the row's
 * cumulative table.  Length table and payloads are therefore byte for byte those of a version-3
 * container packed with the same tables, geometry and L (neighbours = 0: of a version-2 container
 * with K = K0).
 * Fit rule (integers only): a row's counts c_0 .. c_{nsym-1} are taken over the whole stream at
 * the container's L; n_r is their sum.  n_r = 0: f_s = floor(4096*(s+1)/nsym) - floor(4096*s/nsym).
 * Otherwise f_s = 1 + floor(c_s*(4096 - nsym)/n_r) in 64-bit arithmetic, and the deficit
 * 4096 - sum f_s (0 <= deficit < nsym) is added to the symbol with the largest count, the lowest
 * index on ties.
 * The "TICS" entries above reject these containers (another magic), and these reject "TICS". */

/* counts[K0*M][nsym] (overwritten): symbol k of sym[0..n) counts in row (k mod K0)*M + nb at
 * segment length L.  TIC_EINVAL for a symbol >= nsym or a model outside the limits. */
int tic_rcseg_count_nbr(const uint8_t* sym, size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym,
                        uint32_t eh, uint32_t ew, uint32_t C, uint64_t* counts);
/* The fit rule: counts[K][nsym] (each at most 2^40) to cumulative tables[K][nsym + 1], totals 4096. */
int tic_rcseg_fit_tables(const uint64_t* counts, size_t K, size_t nsym, int64_t* tables);
/* tic_rcseg_bound + 20 + T. */
int tic_rcseg_bound_emb(size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym, size_t* bytes);
/* Count, fit, write: the container of sym[0..n).  cap >= tic_rcseg_bound_emb. */
int tic_rcseg_encode_emb(const uint8_t* sym, size_t n, uint32_t L, size_t K0, uint32_t neighbours, size_t nsym,
                         uint32_t eh, uint32_t ew, uint32_t C, uint8_t* out, size_t cap, size_t* written);
/* Validates everything: magic, version, the zero bytes, the limits, T against its formula, the
 * CRC, every frequency >= 1 with row sums <= 4095, and the length table as tic_rcseg_parse does.
 * Outputs may be NULL; tables, when given, receives the K0*M cumulative rows [nsym + 1]. */
int tic_rcseg_parse_emb(const uint8_t* buf, size_t nbytes, uint32_t* L, uint64_t* n, uint32_t* K0, uint32_t* eh,
                        uint32_t* ew, uint32_t* C, uint32_t* neighbours, uint32_t* nsym, int64_t* tables);
/* tic_rcseg_parse_emb, TIC_EINVAL when n differs from the header's, then the n symbols.  No table
 * argument: the container's own. */
int tic_rcseg_decode_emb(const uint8_t* buf, size_t nbytes, uint8_t* sym_out, size_t n);
/* tic_rcseg_range_extent for a "TICA" container; needs only the bytes [0, 40 + T + 2S). */
int tic_rcseg_range_extent_emb(const uint8_t* buf, size_t nbytes, size_t first, size_t count, size_t* j0, size_t* nj,
                               size_t* byte_off, size_t* byte_len);
/* tic_rcseg_decode_range for a "TICA" container; reads no payload byte outside the extent. */
int tic_rcseg_decode_range_emb(const uint8_t* buf, size_t nbytes, uint8_t* sym_out, size_t n, size_t first,
                               size_t count);

/* --- segmented streams on the device (csrc/tic_entropy.cpp) ---
 * One range coder per lane, one segment each; a scan over the segment lengths; a gather that
 * writes the containers.  All entries are asynchronous on the handle's stream, never synchronise,
 * read their HOST arrays (offsets, counts, sizes) during the call only, and run on any handle.
 * Deterministic: no atomic decides an output byte. */

/* The table of the following calls on this handle (validated as the host entries do; replaces
 * the previous one, ordered on the stream).  Totals up to 65536 decode through a value -> symbol
 * table in LDS, larger ones (up to 2^24) through a search of the cumulative table. */
int tic_entropy_set_table(tic_handle* h, const int64_t* cum_freq, size_t ncum);
/* Device scratch (bytes) either device entry needs for streams of these symbol counts at segment
 * length L (decode: the smallest L of the containers).  Host arithmetic only. */
int tic_entropy_scratch_bytes(const int64_t* counts, int n_streams, uint32_t L, size_t* bytes);
/* Stream i: counts[i] symbols at d_sym + sym_offsets[i] (any alignment, order, gaps).  d_out
 * receives the n_streams containers back to back, d_sizes[i] (device, 8-byte aligned) their byte
 * sizes; bytes behind the last container are not written.  A stream with a symbol outside the
 * table gets d_sizes[i] = UINT64_MAX and contributes no bytes.  d_scratch 16-byte aligned.
 * TIC_EINVAL with nothing launched for null pointers, a negative count or offset, counts[i] == 0,
 * a bad L, no table, a scratch below tic_entropy_scratch_bytes or out_cap below the sum of
 * tic_rcseg_bound; n_streams == 0 does nothing. */
int tic_entropy_encode_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts,
                              int n_streams, uint32_t L, void* d_scratch, size_t scratch_bytes, uint8_t* d_out,
                              size_t out_cap, uint64_t* d_sizes);
/* Container i: blob_sizes[i] bytes at d_blob + blob_offsets[i], already passed through
 * tic_rcseg_parse by the caller; its counts[i] symbols go to d_sym + sym_offsets[i].  Whatever
 * the bytes hold, the kernels read only inside the container, clamp segment extents to it and
 * write exactly counts[i] symbols below the table's symbol count (zeros for a container whose
 * header does not fit counts[i], its size or the scratch); for a valid container they equal
 * tic_rcseg_decode's. */
int tic_entropy_decode_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                              const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                              const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);

/* --- version-2 (context) streams on the device ---
 * The K tables of the following *_ctx_device calls on this handle, validated as
 * tic_rcseg_encode_ctx does and uploaded to a device buffer the handle owns (freed by
 * tic_destroy); the upload is ordered on the handle's stream and complete on return.
 * Independent of tic_entropy_set_table: the version-1 entries keep their table.  The coder
 * kernels stage the tables in LDS when K*ncum*4 <= 64 KiB and read them from global memory
 * otherwise. */
int tic_entropy_set_tables(tic_handle* h, const int64_t* tables, size_t K, size_t ncum);
/* tic_entropy_encode_device writing version-2 containers under the tables set: the same
 * arguments, scratch (tic_entropy_scratch_bytes) and contract, out_cap at least the sum of
 * tic_rcseg_bound_ctx.  Every stream starts at context 0. */
int tic_entropy_encode_ctx_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes);
/* tic_entropy_decode_device for version-2 containers (passed through tic_rcseg_parse_ctx by the
 * caller).  A container whose version, K or CRC is not that of the tables set decodes to zeros,
 * as one whose header does not fit counts[i]. */
int tic_entropy_decode_ctx_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);
/* tic_histogram_device per context: symbol i of d_sym[0..n) counts in row i mod K of the uint64
 * counts d_counts[K][Q] (8-byte aligned; accumulates, zero it first; d_sym of any alignment).
 * Integer adds only: the result does not depend on the order they happen in.  1 <= K <= 65536. */
int tic_histogram_ctx_device(tic_handle* h, const uint8_t* d_sym, size_t n, int Q, int K, uint64_t* d_counts);

/* --- version-3 (causal-neighbour) streams on the device ---
 * The K0*M tables, the geometry and `neighbours` of the following *_nbr_device calls on this
 * handle, validated as tic_rcseg_encode_nbr does.  They are uploaded as tic_entropy_set_tables
 * uploads its tables, into the same per-handle buffer (so they replace version-2 tables, and
 * tic_entropy_set_tables replaces them), ordered on the handle's stream and complete on return. */
int tic_entropy_set_tables_nbr(tic_handle* h, const int64_t* tables, size_t K0, uint32_t neighbours, size_t ncum,
                               uint32_t eh, uint32_t ew, uint32_t C);
/* tic_entropy_encode_ctx_device writing version-3 containers: the same arguments and contract,
 * out_cap at least the sum of tic_rcseg_bound_nbr.  Every stream starts at position 0 of a patch.
 * A lane carries (c, w, h) and its K0 phase as counters and reads its neighbours from d_sym. */
int tic_entropy_encode_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes);
/* tic_entropy_decode_ctx_device for version-3 containers (passed through tic_rcseg_parse_nbr by
 * the caller).  A container whose version, K0, CRC, geometry or neighbours is not what was set
 * decodes to zeros.  A lane keeps the classes of its own last symbols as a ring of bits in LDS
 * (as far back as its farthest neighbour that a segment can reach); when the rings of a workgroup
 * exceed 64 KiB it re-reads the bytes it stored itself instead.  No lane reads another's output. */
int tic_entropy_decode_nbr_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);
/* Symbol k of stream i (counts[i] symbols at d_sym + sym_offsets[i]) counts in row
 * (k mod K0)*M + nb of the uint64 counts d_counts[K0*M][Q], nb as the coder derives it at segment
 * length L from the geometry, K0 and neighbours last set on the handle (class(s) = 2*s >= Q;
 * np.histogram's bins as tic_histogram_device).  Accumulates; integer adds only. */
int tic_histogram_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets, const int64_t* counts,
                             int n_streams, int Q, uint32_t L, uint64_t* d_counts);

/* --- symbol ranges of segmented streams on the device ---
 * tic_entropy_decode_device / _ctx_device / _nbr_device for one symbol range per record.  Range r:
 * symbols [firsts[r], firsts[r] + counts[r]) of the container of blob_sizes[r] bytes at d_blob +
 * blob_offsets[r], which holds stream_counts[r] symbols (the header's n), go to d_sym +
 * sym_offsets[r] (any alignment, order and gaps); bytes of d_sym outside the ranges are not
 * written.  Several ranges may name one container.  All six arrays are HOST arrays of n_ranges
 * entries, read during the call only.  For a valid container the symbols equal those of
 * tic_rcseg_decode_range / _ctx / _nbr.  A container whose header does not fit stream_counts[r],
 * its size or what was set on the handle (version, K / K0, CRC, geometry, neighbours) yields
 * zeros for its ranges, as does a range whose segments' payloads would end outside the container.
 * The kernels read the header, the u16 lengths of segments 0 .. j1 and the payloads of segments
 * j0 .. j1 of each range (j0 = first / L, j1 = (first + count - 1) / L), and nothing else of a
 * container: the other bytes need not be on the device.  One segment per lane: a lane decodes its
 * segment from the start, as the chain cannot begin in the middle, up to the range's end, and
 * stores only the symbols inside the range.  Asynchronous on the handle's stream, no
 * synchronisation, no atomics.  TIC_EINVAL with nothing launched for what the entries above
 * reject, and for counts[r] <= 0, firsts[r] < 0 or a range not inside stream_counts[r];
 * n_ranges == 0 does nothing. */

/* Device scratch (bytes) the three entries need for these ranges at segment length L (the
 * smallest L of the containers): room for the most segments a range of counts[r] symbols can
 * touch, wherever it starts.  Host arithmetic only. */
int tic_entropy_ranges_scratch_bytes(const int64_t* firsts, const int64_t* counts, int n_ranges, uint32_t L,
                                     size_t* bytes);
int tic_entropy_decode_ranges_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                     const int64_t* blob_sizes, const int64_t* stream_counts, const int64_t* firsts,
                                     const int64_t* counts, int n_ranges, uint8_t* d_sym, const int64_t* sym_offsets,
                                     void* d_scratch, size_t scratch_bytes);
int tic_entropy_decode_ranges_ctx_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, uint8_t* d_sym,
                                         const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);
/* Version 3: where the class rings of 64 lanes do not fit 64 KiB of LDS, 32 lanes of a workgroup
 * work, each with its ring in LDS (a lane cannot re-read symbols it did not store). */
int tic_entropy_decode_ranges_nbr_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, uint8_t* d_sym,
                                         const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);

/* --- "TICA" streams on the device (csrc/tic_entropy_emb.cpp) ---
 * One model (K0, neighbours, nsym, eh, ew, C) per call, tables per stream.  The model comes with
 * every call: no tic_entropy_set_* call is needed and the handle's tables are left alone.  As the
 * entries above: asynchronous on the handle's stream, no call synchronises, HOST arrays are read
 * during the call only, TIC_EINVAL with nothing launched for what the version-3 entries reject and
 * for a model outside the format's limits; n_streams == 0 does nothing.  Deterministic: the
 * counters are integers, and no atomic decides an output byte otherwise. */

/* Symbol k of stream i (counts[i] symbols at d_sym + sym_offsets[i]) counts in row
 * (k mod K0)*M + nb of the uint64 counts d_counts[n_streams][K0*M][nsym] (8-byte aligned), nb as
 * the coder derives it at segment length L.  A symbol >= nsym counts nowhere; as a neighbour its
 * class is 1.  Accumulates (zero the counts first); integer adds only.  A workgroup counts in LDS
 * when a stream's counts fit 32 KiB and adds its counts to the stream's once. */
int tic_histogram_streams_nbr_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                     const int64_t* counts, int n_streams, size_t nsym, uint32_t L, size_t K0,
                                     uint32_t neighbours, uint32_t eh, uint32_t ew, uint32_t C, uint64_t* d_counts);
/* Device scratch (bytes) tic_entropy_encode_emb_device and tic_entropy_decode_emb_device need for
 * streams of these symbol counts at segment length L (decode: the smallest L of the containers).
 * Host arithmetic only. */
int tic_entropy_emb_scratch_bytes(const int64_t* counts, int n_streams, uint32_t L, size_t K0, uint32_t neighbours,
                                  size_t nsym, size_t* bytes);
/* tic_entropy_encode_nbr_device writing "TICA" containers, byte for byte tic_rcseg_encode_emb's:
 * per-stream counts, the fit (one thread per row) and the per-stream cumulative tables live in the
 * scratch; the segment coder reads its stream's tables (every stream gets whole workgroups, which
 * stage the tables in LDS when K0*M*(nsym+1)*4 <= 64 KiB and read them from the scratch
 * otherwise); the gather writes header, table block, CRC, length table and payloads.  out_cap at
 * least the sum of tic_rcseg_bound_emb; d_sizes[i] = UINT64_MAX for a stream with a symbol >= nsym. */
int tic_entropy_encode_emb_device(tic_handle* h, const uint8_t* d_sym, const int64_t* sym_offsets,
                                  const int64_t* counts, int n_streams, uint32_t L, size_t K0, uint32_t neighbours,
                                  size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, void* d_scratch,
                                  size_t scratch_bytes, uint8_t* d_out, size_t out_cap, uint64_t* d_sizes);
/* tic_entropy_decode_nbr_device for "TICA" containers.  Every header is checked against the
 * model given, counts[i] and blob_sizes[i], and the cumulative tables are rebuilt from the table
 * block into the scratch.  A container that disagrees decodes to zeros, as one whose table block
 * has a zero frequency or a row sum above 4095, fails its CRC or does not lie inside
 * blob_sizes[i].  Reads stay inside each container whatever it holds; exactly counts[i] symbols
 * below nsym are written. */
int tic_entropy_decode_emb_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                  const int64_t* blob_sizes, const int64_t* counts, int n_streams, size_t K0,
                                  uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C, uint8_t* d_sym,
                                  const int64_t* sym_offsets, void* d_scratch, size_t scratch_bytes);
/* tic_entropy_ranges_scratch_bytes / tic_entropy_decode_ranges_nbr_device for "TICA" containers:
 * one range per record (every record rebuilds its container's tables).  Only the bytes
 * [0, 40 + T + 2S) of a container and the payloads of the range's segments are read. */
int tic_entropy_ranges_emb_scratch_bytes(const int64_t* firsts, const int64_t* counts, int n_ranges, uint32_t L,
                                         size_t K0, uint32_t neighbours, size_t nsym, size_t* bytes);
int tic_entropy_decode_ranges_emb_device(tic_handle* h, const uint8_t* d_blob, const int64_t* blob_offsets,
                                         const int64_t* blob_sizes, const int64_t* stream_counts,
                                         const int64_t* firsts, const int64_t* counts, int n_ranges, size_t K0,
                                         uint32_t neighbours, size_t nsym, uint32_t eh, uint32_t ew, uint32_t C,
                                         uint8_t* d_sym, const int64_t* sym_offsets, void* d_scratch,
                                         size_t scratch_bytes);

/* --- a region of an image (csrc/tic_region.cpp) ---
 * Patches are independent and, in a segmented stream, so are the symbols of different segments:
 * the rectangle [y, y + h) x [x, x + w) of an H x W image can be decoded from the patches it
 * needs.  The patches py0 <= py < py1, px0 <= px < px1 of the image's grid, row-major, are the
 * patch batch of an image of the box's size (the box clipped to H x W), so the decoder,
 * tic_patches_to_images_device and tic_round_u8_device serve them unchanged; for every grid row
 * of the box the patches px0 .. px1 - 1 are one contiguous symbol range of the stream
 * (tic_entropy_decode_ranges*_device). */

/* The patch box of a region.  S = 0: no post-filter, the box is the patch rows and columns the
 * region touches.  S > 0 (even; 128 for the rmbe net): the region is first widened, per axis, over
 * every window band of the post-filter's second pass it intersects, then over every band of the
 * first pass the result intersects, with o = S / 2:
 *   rows     pass 2: [o + a*S, o + a*S + S), a < (H - o) / S;  pass 1: [a*S, a*S + S), a < H / S
 *   columns  pass 2: [b*S, b*S + S), b < W / S;                pass 1: [o + b*S, ...), b < (W - o) / S
 * then aligned to P and clipped to the patch grid.  That is a superset of what the region's pixels
 * depend on: a pixel's pass-2 window lies in the box, every pixel of that window has its pass-1
 * window in the box, and further windows inside the box touch no pixel of the region, because the
 * windows of one pass are disjoint.  The box exceeds the region's own patch box by less than
 * 2*S + P pixels per side.  Host arithmetic: no device, no handle.  TIC_EINVAL for a region that
 * is empty or not inside H x W, P <= 0 or a bad S. */
int tic_region_plan(int H, int W, int P, int y, int x, int h, int w, int S, int* py0, int* py1, int* px0, int* px1);

/* tic_rmbe_images_device on parts of images.  Region i is a float32 HWC block of heights[i] x
 * widths[i] at offsets[i] (floats) of the arena and holds rows y0s[i].. and columns x0s[i].. of an
 * image of full_heights[i] x full_widths[i].  Filters, in place, every first-pass window of the
 * FULL image's grid (positions and counts as tic_rmbe_image_device for the full size, not the
 * region's) that lies wholly inside the region, then every such second-pass window; pixels in no
 * such window stay untouched.  One gather, one run of the network and one write-back per pass for
 * the whole list.  A region at origin (0, 0) with the full size gives tic_rmbe_image_device's
 * result bit for bit; a region that is tic_region_plan's box gives the full image's result on the
 * pixels the box was planned for.  HOST arrays of n entries, read during the call only.
 * TIC_MODEL_RMBE handle; TIC_EINVAL for a region not inside its image or overlapping regions. */
int tic_rmbe_regions_device(tic_handle* h, float* d_arena, const int64_t* offsets, const int32_t* heights,
                            const int32_t* widths, const int32_t* y0s, const int32_t* x0s,
                            const int32_t* full_heights, const int32_t* full_widths, int n);

/* Crop i: rows [ys[i], ys[i] + hs[i]) x columns [xs[i], xs[i] + ws[i]) of the uint8 HWC box of
 * heights[i] x widths[i] at byte offsets[i] of d_boxes, as a dense [hs[i], ws[i], 3] block at byte
 * out_offsets[i] of d_out (one launch for the list; bytes of d_out in no block are not written).
 * Any handle.  TIC_EINVAL for a crop not inside its box or overlapping outputs. */
int tic_crop_regions_device(tic_handle* h, const uint8_t* d_boxes, const int64_t* offsets, const int32_t* heights,
                            const int32_t* widths, const int32_t* ys, const int32_t* xs, const int32_t* hs,
                            const int32_t* ws, const int64_t* out_offsets, int n, uint8_t* d_out);

#ifdef __cplusplus
}
#endif

#endif /* TIC_H_ */
