/*
 * wavernn_amd.h — C-ABI of the MI355X-native WaveRNN generation path.
 *
 * The reference has no FFI: its hot path is the Python method
 *   WaveRNN.generate(mels, save_path, batched, target, overlap, mu_law)
 *   (/root/reference/models/fatchord_version.py:169-264)
 * whose per-sample loop (:201-241) dispatches ~40 eager torch ops per step.  This ABI is
 * what that method binds instead (wavernn_amd/fatchord_version.py does it via ctypes; see
 * INTEGRATION.md for the binding a reference maintainer would add).  Each entry point names
 * the reference code it replaces.
 *
 * Conventions: plain pointers and sizes only; return 0 or a negative WRNN_E* code; no
 * exception crosses the ABI; device pointers are HIP device pointers on the handle's device;
 * `stream` is a hipStream_t (NULL = default stream); calls are asynchronous on that stream
 * except where stated; one handle per device, not thread-safe.
 */
#ifndef WAVERNN_AMD_H
#define WAVERNN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WRNN_ABI_VERSION 7

enum wrnn_status {
    WRNN_OK = 0,
    WRNN_EINVAL = -1,        /* bad argument / shape (message in wrnn_last_error)            */
    WRNN_EHIP = -2,          /* a HIP runtime call failed                                    */
    WRNN_ENOWEIGHTS = -3,    /* wrnn_generate before every required tensor was set           */
    WRNN_ETIMEOUT = -4,      /* a persistent-kernel wait exceeded its bound (kernel aborted)  */
    WRNN_ENOMEM = -5,
    WRNN_EUNSUPPORTED = -6,  /* dims / device the kernel cannot run (e.g. LDS or residency)  */
};

enum wrnn_mode {             /* fatchord_version.py:97-104 */
    WRNN_MODE_RAW = 0,       /* softmax over 2**bits classes, Categorical sample (:231-237) */
    WRNN_MODE_MOL = 1,       /* 30-way mixture of logistics (:225-229)                       */
    WRNN_MODE_DM = 2,        /* deepmind_version.py: dual coarse/fine 8-bit softmax (:75-165);
                                rnn_dims = hidden_size, n_classes = quantisation; the fc/aux/
                                feat dims are unused (no conditioning)                         */
};

typedef struct wrnn_ctx wrnn_t;

/* Model dims — the WaveRNN constructor arguments that shape the loop
 * (fatchord_version.py:93-123; aux_dims = res_out_dims / 4 at :110). */
typedef struct {
    int32_t abi_version;     /* must be WRNN_ABI_VERSION */
    int32_t mode;            /* enum wrnn_mode */
    int32_t rnn_dims;
    int32_t fc_dims;
    int32_t aux_dims;
    int32_t feat_dims;       /* num_mels */
    int32_t n_classes;       /* 2**bits (RAW) or 30 (MOL) */
    int32_t grid;            /* workgroups of the persistent kernel; 0 = auto (one per CU) */
    int32_t timeout_ms;      /* bound on any single in-kernel wait; 0 = default (2000 ms) */
} wrnn_config;

/* One named weight, named exactly as the reference state_dict key
 * (e.g. "rnn1.weight_ih_l0"), fp32 row-major in the reference shape. */
typedef struct {
    const char *name;
    const float *data;
    int64_t numel;
    int32_t on_device;       /* 1: `data` is a device pointer, 0: host pointer */
} wrnn_tensor;

/* Launch geometry chosen for the handle (read-only).  Kernels: the XCD-resident kernel (MoL
 * rnn/fc 512, up to 8 rows per launch, one row on each XCD's 32 CUs), its many-row form (up to
 * 16 rows per XCD on the matrix cores, 128 per launch), the role-split kernel
 * (one MoL row), the per-row latency kernel (rows in LDS, used while B <= max_rows) and the
 * multi-row kernel (rows through HBM). */
typedef struct {
    int32_t grid;            /* workgroups (all co-resident, one persistent launch) */
    int32_t units_rnn;       /* hidden units per workgroup (GRU rows ×3)            */
    int32_t units_fc;        /* fc1/fc2 rows per workgroup                          */
    int32_t units_cls;       /* fc3 rows per workgroup (RAW; MOL computes all 30)   */
    int32_t max_rows;        /* rows one latency-kernel launch holds (0: multi-row kernel only) */
    int32_t lds_bytes;       /* dynamic LDS per workgroup at max_rows                */
    int32_t slab_floats;     /* resident weight floats per workgroup                 */
    int32_t num_cus;
    int32_t rows_grid;       /* multi-row kernel: workgroups (0: unavailable)        */
    int32_t rows_units_rnn;  /*                   hidden units per workgroup         */
    int32_t sparse_blocks;   /*                   max nonzero 4x4 blocks per gate block-row when
                                                  the GRU weights are block-sparse, else 0 */
    int32_t split_grid;      /* batch-1 MoL role-split kernel: GRU + FC workgroups (0: unavailable) */
    int32_t last_path;       /* kernel of the last wrnn_generate: 1 latency, 2 multi-row,
                                3 deepmind, 4 role-split, 5 XCD-resident, 6 XCD-resident
                                block-sparse rnn 896, 7 XCD-resident many-row, 8 XCD-resident
                                deepmind, 9 multi-row with the weights streamed from HBM (dense
                                weights beyond LDS), 10 deepmind streamed (0: none yet) */
    int32_t xcd_rows;        /* XCD-resident kernel, rows per launch (0: unavailable).  RAW/MOL
                                handles: the one-row-per-XCD kernel (dense rnn 512, or rnn 896
                                with block-sparse GRU weights once they are set), 8.  DM handles
                                (ABI 5): the XCD-resident deepmind kernel (hidden 896 / Q 256,
                                4 rows per XCD), 32. */
    int32_t xcdm_rows;       /* XCD-resident many-row kernel (MoL rnn/fc 512): rows per launch
                                (0: unavailable)                                           (ABI 5) */
    /* What the last multi-row call chose (ABI 7): wrnn_generate on the multi-row or the deepmind rows
       kernel (last_path 2, 9, 3, 10) or a rows session's push.  All 0 after any other call. */
    int32_t last_row_groups; /* 1, or 2: the rows of a block in two groups on half the workgroups each */
    int32_t last_row_blocks; /* row blocks (launch loops of <= 256 rows) the call ran                */
    int32_t last_block_rows; /* rows of its first block, after any shrink to what LDS holds          */
    int32_t last_tile_rows;  /* rows per register tile (TB) of its first block                       */
} wrnn_info;

/* Create a handle on `device` (replaces WaveRNN.__init__ for the loop's dims,
 * fatchord_version.py:93-129).  Synchronous.  On failure *out may still hold a handle so
 * the caller can read wrnn_last_error(); release it with wrnn_destroy. */
int wrnn_create(const wrnn_config *cfg, int device, wrnn_t **out);

/* Load weights by reference state_dict name (replaces WaveRNN.load → load_state_dict,
 * fatchord_version.py:414-417, for the loop's tensors: I.*, rnn1.*, rnn2.*, fc1-3.*).
 * Copies and packs into the kernel's per-workgroup layout; the caller keeps ownership.
 * Unknown names are ignored (load_state_dict(strict=False)).  Synchronous.
 * May be called again on a live handle, with all tensors or some: every slab is repacked and
 * every layout decision taken again (block density <= 1/2: the sparse rows layout where its slab
 * fits beside one row of state, else the dense one, resident or streamed).  Streaming sessions
 * opened before the call are refused from then on (wrnn_stream_push). */
int wrnn_set_weights(wrnn_t *h, const wrnn_tensor *tensors, int n);

/* Run the whole sample loop (fatchord_version.py:192-241) for B rows × L steps.
 *   cond   [L][B][feat_dims + 4·aux_dims]  upsampled mel ‖ aux, time-major (device);
 *          NULL in DM mode (deepmind_version.generate(seq_len) has no conditioning)
 *   noise  [L][B][K] injected draws in reference order, or NULL for in-kernel Philox:
 *          MOL K = 11 (u1[10], u2 ∈ (1e-5, 1−1e-5), utils/distribution.py:106,118);
 *          RAW K = n_classes (q ~ Exp(1); Categorical.sample ≡ argmax(probs/q));
 *          DM  K = 2·n_classes (q_coarse, then q_fine, deepmind_version.py:130,150)
 *   seed, row_offset  Philox key and global id of row 0 (draws are keyed by
 *          (seed, row_offset + b, step, k), so sharding rows across calls/GPUs is invariant)
 *   out    [B][L] fp32 samples (the values appended at :227/:236; DM: the combined 16-bit
 *          sample coarse·256 + fine − 2^15, utils/dsp.py:33-34)               (device)
 *   labels [B][L] int32 class labels (RAW) / combined samples (DM), or NULL  (device)
 * Asynchronous on `stream`; kernel-side failures surface through wrnn_check. */
int wrnn_generate(wrnn_t *h, const float *cond, int B, int L, const float *noise,
                  uint64_t seed, int64_t row_offset, float *out, int32_t *labels, void *stream);

/* Synchronise `stream` and report a persistent-kernel abort (WRNN_ETIMEOUT) from the
 * last wrnn_generate on it.  The reference raises synchronously; this is that check. */
int wrnn_check(wrnn_t *h, void *stream);

/* Device time (ms, HIP events on the launch stream) from the first to the last persistent
 * loop launch of the last wrnn_generate — the kernel time the roofline is computed from.
 * Waits for that launch to finish. */
int wrnn_elapsed_ms(wrnn_t *h, float *ms);

int wrnn_query(const wrnn_t *h, wrnn_info *info);
const char *wrnn_last_error(const wrnn_t *h);
void wrnn_destroy(wrnn_t *h);

/* ---- conditioning producer and waveform consumer (stateless; no handle) ----------------- */

/* The UpsampleNetwork's mel path: per scale s_i a nearest Stretch2d(s_i) and a Conv2d(1,1,
 * (1, 2·s_i+1), padding (0, s_i), no bias) whose taps are `upsample.up_layers.{2i+1}.weight`
 * (fatchord_version.py:64-79), applied to the mel zero-padded by `pad` frames each side. */
typedef struct {
    int32_t feat_dims;       /* num_mels (80) */
    int32_t res_out_dims;    /* MelResNet output channels (128) = 4·aux_dims */
    int32_t pad;             /* voc_pad (2) */
    int32_t n_scales;        /* 1..4 (hparams voc_upsample_factors = (5, 5, 11)) */
    int32_t scales[4];       /* each 1..15 */
    const float *taps[4];    /* HOST pointers, 2·scales[i]+1 floats each */
} wrnn_upsample_cfg;

/* Shape of the conditioning wrnn_upsample_pack writes for `B` mel rows of `T` frames:
 * steps = L = hop·T unbatched (target <= 0), else the fold window target + 2·overlap;
 * rows = B·num_folds (fold_with_overlap, fatchord_version.py:317-330). */
int wrnn_cond_shape(const wrnn_upsample_cfg *cfg, int B, int T, int target, int overlap,
                    int *steps, int *rows);

/* Replaces, in one kernel, everything between MelResNet and the loop's input
 * (fatchord_version.py:183-205): pad_tensor(pad) → 3× (Stretch2d, Conv2d) → crop indent (:88)
 * for the mel, resnet_stretch (:83) for `aux`, fold_with_overlap (:293-340, target <= 0:
 * unbatched) and the cat/transpose into the time-major records wrnn_generate reads.
 *   mel   [B][feat_dims][T]     the generate() input (device, fp32)
 *   aux   [B][res_out_dims][T]  MelResNet(pad_tensor(mel)) output (device, fp32)
 *   cond  [steps][rows][feat_dims + res_out_dims]  (device; row = b·num_folds + fold) */
int wrnn_upsample_pack(const wrnn_upsample_cfg *cfg, const float *mel, const float *aux, int B, int T,
                       int target, int overlap, float *cond, void *stream);

/* wrnn_upsample_pack's unbatched records for a WINDOW of steps of an utterance still arriving
 * (window addition, same ABI): steps [t0, t0 + n) of U utterances.
 *   mel   [U][feat_dims][nm]     frames [m0, m0 + nm)      (device, fp32)
 *   aux   [U][res_out_dims][na]  frames [a0, a0 + na)      (device, fp32)
 *   T     the utterance's frame count, or −1 while it is unknown
 *   cond  [n][U][feat_dims + res_out_dims]: record of step t0 + i at row i
 * Frames outside [0, T) are zeros (pad_tensor); while T is −1 nothing lies past the end.  Every record
 * equals, bit for bit, the one wrnn_upsample_pack writes for that step of the whole utterance: the
 * same kernel body, the same 3-point stencil per level in the same fmaf order.
 * WRNN_EINVAL before any launch when a window lacks a frame the steps read
 * (wrnn_upsample_window_frames), or the steps reach past hop·T. */
int wrnn_upsample_pack_window(const wrnn_upsample_cfg *cfg, const float *mel, int m0, int nm, const float *aux, int a0,
                              int na, int T, int U, int t0, int n, float *cond, void *stream);

/* The frames wrnn_upsample_pack_window reads for steps [t0, t0 + n) (host only, stateless): mel
 * frames [*mel_lo, *mel_hi) and aux frames [*aux_lo, *aux_hi), clipped to [0, T) when T >= 0. */
int wrnn_upsample_window_frames(const wrnn_upsample_cfg *cfg, int T, int t0, int n, int *mel_lo, int *mel_hi,
                                int *aux_lo, int *aux_hi);

/* wrnn_upsample_pack + wrnn_generate in one call, from the generate() inputs at FRAME rate
 * (ABI 6): mel [U][feat_dims][T] and aux [U][res_out_dims][T] (MelResNet of the padded mel) for U
 * utterances of T frames each; rows / steps as wrnn_cond_shape (target <= 0: unbatched, row u =
 * utterance u; else utterance u's folds are rows u·nf .. u·nf + nf − 1).  noise, seed, row_offset,
 * out, labels as wrnn_generate.
 * The UpsampleNetwork is linear and frame-shift-invariant, so on the XCD-resident paths the
 * conditioning terms W·[mel_up | aux | 1] are formed as W·(frames) — a GEMM over T frames instead
 * of hop·T samples — plus a per-sample sum of ≤ 8 frame rows weighted by the stretch/conv
 * cascade's response (csrc/frame_terms.hip); the other paths get wrnn_upsample_pack's records.
 * Replaces fatchord_version.py:183-241 (pad → upsample → fold → sample loop). */
int wrnn_generate_frames(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *mel, const float *aux, int U, int T,
                         int target, int overlap, const float *noise, uint64_t seed, int64_t row_offset, float *out,
                         int32_t *labels, void *stream);

/* wrnn_generate_frames for the loop rows [row_begin, row_begin + row_count) of that launch only
 * (round-5 addition, same ABI): e.g. a contiguous block of one long utterance's folds on one GPU
 * of a node (wavernn_amd/sharding.py generate_sharded_folds).  The rows keep their
 * place in the utterance (row r = fold r % nf of utterance r / nf); noise [steps][row_count][K],
 * out / labels [row_count][steps]; row_offset keys the Philox draws of launch row j as
 * row_offset + j (pass the global row id of row_begin). */
int wrnn_generate_frames_rows(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *mel, const float *aux, int U,
                              int T, int target, int overlap, int row_begin, int row_count, const float *noise,
                              uint64_t seed, int64_t row_offset, float *out, int32_t *labels, void *stream);

/* The frame weights wrnn_generate_frames uses (host, stateless): mel_up(p) = Σ_k coef[φ][k] ·
 * mel[f + k + jlo] for p = f·hop + φ, 0 <= k < nJ — the Stretch2d/Conv2d cascade's response to
 * one frame, float64 rounded to fp32.  coef (nullable) [hop][nJ], coef_cap floats.
 * WRNN_EUNSUPPORTED when pad frames do not cover the response's reach or nJ > 8. */
int wrnn_frame_weights(const wrnn_upsample_cfg *ucfg, int *hop, int *nJ, int *jlo, float *coef, int coef_cap);

/* The UpsampleNetwork's MelResNet (fatchord_version.py:13-48) in inference form, one kernel:
 * conv_in (k = 2·pad + 1) → BN → ReLU → res_blocks × [1×1 conv → BN → ReLU → 1×1 conv → BN →
 * + residual] → conv_out, each BatchNorm (running statistics) folded into its conv on the host.
 *   packed [wrnn_melresnet_floats(cfg)] (device): conv_in W[(c·K + tap)][C] + bias[C], per block
 *          W1[C][C] + b1[C] + W2[C][C] + b2[C], conv_out W[C][R] + bias[R] (k-major matrices)
 *   mel    [U][in_dims][T + 2·pad]  pad_tensor'd mel (device);  aux [U][R][T] (device)
 * WRNN_EUNSUPPORTED for channel counts the kernel's thread layout does not cover. */
typedef struct {
    int32_t in_dims;         /* num_mels (80) */
    int32_t compute_dims;    /* C (128) */
    int32_t res_out_dims;    /* R (128) */
    int32_t res_blocks;      /* 10 */
    int32_t pad;             /* voc_pad (2): conv_in kernel 2·pad + 1 */
} wrnn_melresnet_cfg;
int wrnn_melresnet_floats(const wrnn_melresnet_cfg *cfg);
int wrnn_melresnet(const wrnn_melresnet_cfg *cfg, const float *packed, const float *mel, int U, int T, float *aux,
                   void *stream);
/* The frames per workgroup tile wrnn_melresnet takes for U utterances of T frames on the current
 * device (round-6 addition, same ABI): 16, or 4 when a 16-frame grid has fewer workgroups than the
 * device has CUs (both forms sum every output in the same order: bit-identical); channel counts
 * that only one form runs take that form whatever the grid, so support never depends on U·T;
 * negative WRNN_E* as wrnn_melresnet would return. */
int wrnn_melresnet_tile_frames(const wrnn_melresnet_cfg *cfg, int U, int T);

/* generate()'s float64 post-processing on the device (fatchord_version.py:243-258):
 * decode_mu_law (utils/dsp.py:98-103, mu = n_classes) when `mu_law`, xfade_and_unfold
 * (:342-405) of the `rows` folds when `batched` (else row 0), trim to wave_len, and
 * output[-fade_len:] *= linspace(1, 0, fade_len) (fade_len = 20·hop_length).
 *   y     [rows][steps] fp32 loop output (device);  wave [wave_len] float64 (device)
 * WRNN_EINVAL when fade_len > wave_len (the reference's numpy broadcast error, T < 21). */
int wrnn_postprocess(const float *y, int rows, int steps, int batched, int overlap, int mu_law,
                     int n_classes, int wave_len, int fade_len, double *wave, void *stream);

/* Content fingerprints of n device tensors of 32-bit elements (same ABI): out[i] (device, 64 bits
 * each) = sum over j of (bits of element j + 1) * m(j) modulo 2^64, m(j) = splitmix64(j) | 1.
 * Exact integer arithmetic, so a change of any single element changes out[i].  One launch per 64
 * tensors, asynchronous on `stream`.  The drop-in modules key their packed-weight caches on it:
 * an in-place update through `.data` leaves a tensor's pointer and version counter as they were. */
int wrnn_fingerprint(const void *const *tensors, const int64_t *numel, int n, uint64_t *out, void *stream);

/* The sampler draws wrnn_generate takes when noise == NULL, materialised (round-6 addition, same
 * ABI): out [steps][rows][K] (device fp32) = draw k of launch row j at step step0 + s, keyed
 * (seed, row_offset + j, step0 + s, k) exactly as every loop kernel keys its in-kernel Philox, so
 * passing `out` as `noise` reproduces the noise == NULL audio.  Philox-4x32-10 (Salmon et al.,
 * SC'11), counter (k >> 2, step, row lo, row hi), key (seed lo, seed hi), word k & 3; the top 24
 * bits m of the word map to
 *   MOL (K = 11: u1[10], u2; utils/distribution.py:106,118): fma(1 − 2e-5, m·2^-24, 1e-5) in fp32,
 *       i.e. U(1e-5, 1 − 1e-5);
 *   RAW (K = n_classes) and DM (K = 2Q: q_coarse then q_fine): −log((m + 1)·2^-24), i.e. Exp(1)
 *       (Categorical.sample ≡ argmax(probs / q), fatchord_version.py:232-235,
 *       deepmind_version.py:130,150).
 * Restated in numpy by oracle/philox.py (tests/test_philox.py, tests/test_gpu_philox.py). */
int wrnn_philox_draws(uint64_t seed, int64_t row_offset, int rows, int step0, int steps, int K, int mode, float *out,
                      void *stream);

/* ---- streaming synthesis (round-7 addition, same ABI) -------------------------------------
 * Push mel frames as the acoustic model produces them, pull float64 audio as soon as it is final.
 * What generate(mels, None, False, …) computes, unbatched MoL, in pieces: the recurrent state stays
 * on the GPU between calls, the persistent kernel is relaunched per push from that state, and the
 * conditioning terms are formed at frame rate over a window of the running mel.
 *
 * Emission rule.  A sample of frame f reads mel frames up to f + pad (its aux frame, a MelResNet
 * window of ±pad frames; the upsampling cascade reaches no further, wrnn_frame_weights), and a
 * launch that ends before the utterance does also reads the conditioning of the one step after
 * its last, which falls into the next frame.  Hence
 *     lookahead = pad + 1 frames                                  (wrnn_stream_lookahead)
 * and with R frames received and the end not yet seen
 *     steps_done = max(0, R − lookahead) · hop
 *     audio_done = min(steps_done, (T − 1) · hop)                 when total_frames = T was given
 *                = min(steps_done, max(0, (R − 21) · hop))        when the total is unknown: the
 *                  fade-out covers the last 20·hop of the (T − 1)·hop samples, and T >= R
 * both functions of R alone, not of how the frames were chunked.  `final` (R = T) runs the loop to
 * T·hop steps, as generate() does, and releases the rest: audio_done = (T − 1)·hop, the positions
 * inside the last 20·hop multiplied by the same linspace(1, 0, 20·hop) element as wrnn_postprocess.
 * WRNN_EINVAL: final with T < 21 (as wrnn_postprocess), or T != total_frames when that was given. */
typedef struct wrnn_stream wrnn_stream_t;

/* Open a session of U = 1..8 utterances advancing in lock step (one per XCD) on handle `h`.
 *   ucfg, mcfg        the UpsampleNetwork's cascade and MelResNet (copied; taps are host pointers)
 *   melresnet_packed  wrnn_melresnet's packed weights (device; the caller keeps them alive and
 *                     unchanged until wrnn_stream_close)
 *   total_frames      T when known up front, else −1
 *   noise             [noise_steps][U][11] injected draws by absolute step (device; kept by the
 *                     caller until close), or NULL for in-kernel Philox keyed (seed, row_offset + u,
 *                     absolute step) — the draws a one-shot wrnn_generate_frames takes
 * The session owns its recurrent state, hand-off tags, frame-term stores and mel tail: one-shot
 * calls and other sessions on the same handle may run between its pushes, IN STREAM ORDER ON ONE
 * STREAM — the handle's control words, membership counters and rocBLAS stream are shared and
 * every persistent launch fills all XCDs, so work of one handle on two streams at once races (and
 * two persistent grids would wait for each other).  Close every session before wrnn_destroy(h).
 * Synchronous.
 * WRNN_EUNSUPPORTED (message in wrnn_last_error(h)) unless U rows of this handle run on the dense
 * one-row XCD kernel (last_path 5) or the block-sparse rnn-896 one (6), wrnn_frame_weights accepts
 * the cascade and wrnn_melresnet the channel counts. */
int wrnn_stream_open(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                     const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                     uint64_t seed, int64_t row_offset, wrnn_stream_t **out);

/* Append n >= 0 mel frames and write the audio that became final.
 *   mel   [U][feat_dims][n] (device; may be NULL when n = 0)
 *   final nonzero: these are the last frames (n = 0, final = 1 flushes)
 *   wave  [U][cap] float64 (device): utterance u's new samples at wave[u·cap .. u·cap + *n_out)
 *   n_out samples per utterance written by this push = the growth of audio_done above: known on
 *         return, without synchronising (wrnn_stream_plan gives it in advance; cap >= it)
 * Queues its work on `stream` (one stream per handle, see wrnn_stream_open) and does not wait for
 * it, EXCEPT when a session workspace has to grow: the workspaces are sized by the largest push
 * so far (frame records, terms of n·hop + 1 steps, the held-back sample window, the frame-term
 * stores) and growing one frees and reallocates it, which waits for the device.  A session fed
 * pushes of at most the size of its first ones settles after a few pushes (the stores double);
 * a larger push later synchronises once more.
 * Kernel aborts surface through wrnn_check(h, stream); sets wrnn_info.last_path (5 or 6; a wide
 * session, wrnn_stream_open_wide: 7) and leaves wrnn_elapsed_ms at the last wrnn_generate's launch
 * (a wide session sets it to the loop share of the push).  Argument errors (WRNN_EINVAL:
 * counts against the rule above, cap, injected draws too short) are found before anything is
 * queued and leave the session unchanged; any failure after that point kills the session
 * (every later push returns WRNN_EINVAL: close it).
 * A session binds the weights the handle held at wrnn_stream_open: after any later
 * wrnn_set_weights on the handle a push (alone or as a group member) returns WRNN_EINVAL with
 * that cause and the session is dead; other sessions and one-shot calls are unaffected. */
int wrnn_stream_push(wrnn_stream_t *s, const float *mel, int n, int final, double *wave, int cap, int *n_out,
                     void *stream);

/* Advance `count` sessions of ONE handle, each by its own frames, as wrnn_stream_push would one
 * after another on `stream` — but with one persistent launch per time chunk for all of them
 * (group-push addition, same ABI).  A session's utterances advance in lock step: the same frames in
 * the same push, one total_frames, one end.  A group lifts that between sessions: requests that
 * arrived at different times, have different lengths and receive frames at different moments share
 * the GPU, each row on its own XCD over its own step window.
 *   sessions [count]  members: sessions of any U on the same handle (and so the same loop kernel),
 *                     their rows together <= 8 (all of them wide sessions, wrnn_stream_open_wide:
 *                     <= 128), none listed twice, none NULL
 *   mel      [count]  member i's [U_i][feat_dims][n_i] (device), or NULL where n_i = 0 (the array
 *                     itself may be NULL when every n_i = 0)
 *   n, final [count]  as wrnn_stream_push, per member: different totals, different frames received
 *                     so far and different final flags are the normal case
 *   wave, cap, n_out [count]  member i's [U_i][cap_i] float64 (device) and its sample count
 * For every member the result is what wrnn_stream_push(sessions[i], mel[i], n[i], final[i],
 * wave[i], cap[i], &n_out[i], stream) produces: the same emission rule, the same n_out, the same
 * samples.  Each member's conditioning (mel window, MelResNet, frame-term rows, the terms of its
 * steps) runs as in a single push; then launch round j runs time chunk j of every member that
 * still has one, member i's rows on the XCDs after those of the members before it.  The grouped
 * instantiation of the kernel runs the same arithmetic per row in the same order, no hand-off
 * crosses XCDs, so the audio is bit-identical to the session pushed alone on the same schedule.
 * A member whose push makes no step runnable (n = 0, or still inside its look-ahead) takes no XCD;
 * if no member has a step to run no persistent launch is queued, the conditioning and post work of
 * each member still happens.  The WRNN_TERMS_MB budget is shared by all rows with steps to run:
 * a round takes floor(budget / (rows * N) - 1) steps of each, members with fewer steps drop out of
 * the later rounds.
 * Arguments are checked for EVERY member before anything is queued for any of them: count >= 1,
 * the entries above, and per member the checks of wrnn_stream_push (counts against the emission
 * rule, cap, injected draws long enough, not dead, not finished).  On WRNN_EINVAL (message in
 * wrnn_last_error, prefixed "member i: " for a member's own check) every member is unchanged and
 * usable, every n_out is 0.  A failure after queuing has begun kills every member of the group, as
 * a failed single push kills its session.
 * Ordering as wrnn_stream_open states: one stream per handle; one-shot calls, single pushes and
 * other group pushes may run between two group pushes in stream order.  Sets wrnn_info.last_path
 * (5 or 6) when a persistent launch was queued and leaves wrnn_elapsed_ms alone.  Asynchronous
 * except where a member's workspace must grow, as wrnn_stream_push. */
int wrnn_stream_push_group(wrnn_stream_t *const *sessions, int count, const float *const *mel, const int *n,
                           const int *final, double *const *wave, const int *cap, int *n_out, void *stream);

/* ---- Wide sessions: up to 128 session rows per push (wide-group addition, same ABI) ---------
 * wrnn_stream_open with the same arguments, but the session runs on the many-row XCD kernel (16
 * rows per XCD, the weights as register-resident MFMA operands; wrnn_info.last_path 7) and U may be
 * 1..128.  wrnn_stream_push, wrnn_stream_push_group, wrnn_stream_plan and wrnn_stream_close take it
 * like any other session: the same emission rule and look-ahead, the same argument checks and
 * atomic refusals, the same weight binding.  A group whose members are all wide may hold up to 128
 * rows; a group that mixes wide and narrow members is refused ("runs another loop kernel than
 * member 0"); narrow groups keep their limit of 8.  The members of a wide group share one upsample
 * cascade (WRNN_EINVAL otherwise: one interpolation launch serves them all).
 *
 * What a wide session promises.  A member's audio does not depend on its company: every wide
 * launch is the four-quad instantiation of the kernel, whatever the row count, in which the batch
 * rows are independent MFMA columns — a row's bits depend neither on how many rows share the
 * launch nor on the XCD and slot it sits in, so a member of a wide group is bit-identical to the
 * same session pushed alone on the same schedule (a wide group of one).  Against the oracle it lies
 * within the project's bound (2e-5 on whole utterances), and with Philox draws it equals
 * wrnn_generate_frames(seed, row_offset) within 1e-5.
 * What it does not promise.  Bit-equality with the same session opened narrow: the kernel differs
 * (MFMA sums are associated differently from the one-row kernel's), both lie within the bound.
 * And the members' conditioning (MelResNet, frame-term GEMMs) still runs once per member per push;
 * callers whose utterances advance in lock step should open ONE wide session of U rows instead.
 *
 * A push cuts the members' runnable steps into rounds at the distinct step counts in ascending
 * order (all rows of one launch run the same number of steps; members that are done drop out
 * between rounds and the rest are compacted: launch row r on XCD r % 8, slot r / 8), and the
 * WRNN_TERMS_MB budget cuts every round into launches of floor(budget / (rows * 4608) - 1) steps,
 * rows = the rows with a step to run in this push.  The per-row recurrent state lives in the
 * session, so a row may sit in another slot in every launch, and nothing the launches leave on the
 * handle is relied on: one-shot calls (their own many-row launches included), narrow sessions and
 * lists may run between pushes in stream order.  A wide push that queues a persistent launch sets
 * wrnn_elapsed_ms to the device time of its loop share (terms interpolation, draws, hop-area resets
 * and persistent launches of all its rounds): the rest of the push is the members' conditioning.
 * WRNN_EUNSUPPORTED (message in wrnn_last_error(h)) unless the handle is MoL rnn / fc 512 with the
 * many-row kernel co-resident at four quads per XCD (wrnn_info.xcdm_rows == 128), and as
 * wrnn_stream_open where the cascade has no frame-rate form or wrnn_melresnet refuses the channels.
 *
 * RAW handles.  A RAW handle (WRNN_MODE_RAW) opens wide sessions too — and only wide ones: the
 * one-row kernels have no softmax head, wrnn_stream_open refuses it as before.  The session runs the
 * grouped instantiation of the many-row kernel's RAW head under the same promises (every launch the
 * four-quad form, a row's bits independent of company and slot); its class labels are those of
 * wrnn_generate on the same draws, bit for bit, and a session returns audio only (a label is
 * recovered from a sample x as (x + 1)·(n_classes − 1) / 2 when mu-law is off).
 *   noise  [noise_steps][U][512] Exp(1) draws by absolute step, the layout wrnn_generate takes
 *          for a RAW handle; NULL: Philox, the rows launch-for-launch those of wrnn_generate(seed,
 *          row_offset + u)
 * The draws of a RAW row-step (512 floats) share the WRNN_TERMS_MB budget with its terms: a round
 * is cut into launches of floor(budget / (rows * (4608 + 512)) - 1) steps.
 * WRNN_EUNSUPPORTED for a RAW handle names the condition that failed: n_classes != 512 (bits != 9),
 * rnn / fc != 512, or no four-quad form of the many-row kernel on this device.  Deepmind handles
 * are refused. */
int wrnn_stream_open_wide(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                          const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                          uint64_t seed, int64_t row_offset, wrnn_stream_t **out);

/* ---- Rows sessions: streaming for any fatchord model (rows-session addition, same ABI) --------
 * wrnn_stream_open with the same arguments, but the session runs on the multi-row kernel
 * (wrnn_info.last_path 2; 9 when the handle streams its weights from HBM) over per-sample
 * conditioning records, as wrnn_generate does for the models no XCD-resident kernel covers: MoL or
 * RAW, any rnn / fc dims and class count the handle was created with.  wrnn_stream_push,
 * wrnn_stream_plan, wrnn_stream_lookahead, wrnn_stream_mu_law and wrnn_stream_close take it like any
 * other session: the same emission rule and look-ahead, the same argument checks and refusals, the
 * same weight binding.  It is opt-in: wrnn_stream_open and wrnn_stream_open_wide accept and refuse
 * what they did.
 *   U      1 up to the rows wrnn_generate runs as ONE row block of the multi-row kernel for this
 *          handle (at most 256; fewer when the rows' state does not fit LDS beside the weights);
 *          WRNN_EINVAL beyond it, the message states the limit
 *   noise  [noise_steps][U][K] by absolute step, K = 11 (MoL) or n_classes (RAW: Exp(1) draws), the
 *          layout wrnn_generate takes; NULL: Philox keyed (seed, row_offset + u, absolute step)
 * A push runs MelResNet on the frames whose aux became computable, writes the records of the newly
 * runnable steps with wrnn_upsample_pack_window and runs them through wrnn_generate's own launch
 * loop for the multi-row kernel (the same partition by row count, tile, hop form and WRNN_TERMS_MB
 * chunking: floor(budget / (U * (terms + GEMM input))) steps per launch).  The session owns its
 * carried state, mel / aux tails and sample window; the handle's hop areas are zeroed at the start
 * of every push, so one-shot calls and other sessions may run between pushes in stream order.  With
 * the same draws a session's samples are those of wrnn_generate on the whole utterance's records.
 * A RAW session returns audio only (a label is (x + 1)·(n_classes − 1) / 2 with mu-law off).
 * wrnn_stream_push_group refuses a rows member (WRNN_EINVAL, every member untouched): the kernel
 * steps all rows of a launch in lock step, so a rows session advances alone.
 * WRNN_EUNSUPPORTED (message in wrnn_last_error(h)): a deepmind handle, a handle without the
 * multi-row kernel, a cascade that reads further ahead than pad + 1 frames, MelResNet channel counts
 * wrnn_melresnet refuses. */
int wrnn_stream_open_rows(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const wrnn_melresnet_cfg *mcfg,
                          const float *melresnet_packed, int U, int total_frames, const float *noise, int noise_steps,
                          uint64_t seed, int64_t row_offset, wrnn_stream_t **out);

/* RAW sessions: mu-law expansion of the emitted samples (RAW-session addition, same ABI).  on != 0:
 * every sample v leaves as sign(v) / mu · ((1 + mu)^|v| − 1), mu = n_classes − 1, in float64, before
 * the fade — wrnn_postprocess's mu_law.  The default is off.  Valid on a RAW session before its
 * first push; WRNN_EINVAL on a MoL session or after a push, the session unchanged and usable. */
int wrnn_stream_mu_law(wrnn_stream_t *s, int on);

/* The round plan of a wide push as a function (host only, stateless): `count` members with
 * steps[i] >= 0 runnable steps and rows[i] >= 1 rows, at most steps_per_launch steps per launch →
 * the number of persistent launches, and for launch j < cap its first launch-local step, its step
 * count and its rows (the surviving members' rows in member order; launch row r sits on XCD r % 8,
 * slot r / 8).  Negative WRNN_E* (message in wrnn_cond_last_error) on bad counts or more than 128 rows. */
int wrnn_wide_plan(const int *steps, const int *rows, int count, int steps_per_launch, int *launch_first,
                   int *launch_steps, int *launch_rows, int cap);

/* The steps per persistent launch a wide push takes (host only, stateless; reads WRNN_TERMS_MB as the
 * push does): `rows` rows with a step to run, the longest member's runnable steps, raw != 0 for a RAW
 * handle → min(longest_steps, floor(budget / (rows * 4608) - 1)) for MoL, floor(budget / (rows *
 * (4608 + 512)) - 1) for RAW, at least 1: the steps_per_launch of wrnn_wide_plan.  Negative WRNN_E*
 * (message in wrnn_cond_last_error) for rows outside 1..128 or longest_steps < 1. */
int wrnn_wide_steps_per_launch(int rows, int longest_steps, int raw);

/* The emission rule as a function (host only, stateless): the counts a session reports after
 * frames_received frames (`final`: they were the last), total_frames as given to open (−1: unknown).
 * Only ucfg's scales and pad are read.  WRNN_EINVAL as wrnn_stream_push. */
int wrnn_stream_plan(const wrnn_upsample_cfg *ucfg, int frames_received, int final, int total_frames,
                     int64_t *steps_done, int64_t *audio_done);

/* lookahead of the rule above for this cascade: pad + 1 (negative WRNN_E* on a bad ucfg). */
int wrnn_stream_lookahead(const wrnn_upsample_cfg *ucfg);

void wrnn_stream_close(wrnn_stream_t *s);

/* ---- Lists: U whole utterances of unequal length in one call (list addition, same ABI) -----
 * A TTS batch: U mels are all there, each a different length, U waveforms go out.  The eight XCDs
 * are eight LANES; each lane runs a queue of utterances back to back without leaving the
 * persistent kernel, so no utterance waits for the longest of a batch and no lane idles while
 * another still has work queued.
 *
 * Schedule (wrnn_list_plan; host only, stateless, deterministic): longest-processing-time-first.
 * The utterances are taken by decreasing frame count (ties: the lower index first) and each goes to
 * the lane with the smallest load so far (ties: the lowest lane); a lane runs its utterances in
 * the order they were assigned.
 *   frames      [U]      frame counts T_i
 *   lane_of     [U]      out: the lane of utterance i
 *   pos_in_lane [U]      out: its place in that lane's queue (0 = first)
 *   lane_frames [lanes]  out: the lane's timeline in frames (the loop runs hop steps per frame:
 *                        × hop for steps; the schedule is the same in either unit)
 * WRNN_EINVAL (message in wrnn_cond_last_error) for U < 1, lanes outside 1..8 or any T_i < 21, the
 * rule wrnn_postprocess enforces.
 *
 * Rounds.  A lane's timeline is the concatenation of its utterances' steps.  Launch round j covers
 * lane-time [j·C, (j+1)·C) on every lane, C = floor(WRNN_TERMS_MB budget / (lanes · N) − 1) steps
 * (N = terms per row and step; at most the longest timeline) — the rounds are cut by the terms
 * budget only, never by utterance boundaries.  Inside a round a lane's window is cut into pieces
 * at utterance boundaries (the tail of A, all of B, the head of C); every piece has its own terms
 * rows, the one look-ahead row included while its utterance goes on, so a round's terms exceed
 * lanes · C rows by one row per piece.  One persistent launch per round; a lane whose timeline has
 * ended takes no XCD in later rounds.  The piece table of all rounds is uploaded once per call:
 * the host does not wait on the stream between rounds.
 *
 * Contract.  out[i] is, bit for bit, what wrnn_generate_frames(h, ucfg, mel[i], aux[i], 1, T[i], 0, 0,
 * noise[i], seed, row_offset + i, out[i], NULL, stream) writes — for every `lanes` and every
 * WRNN_TERMS_MB.  Utterance i is Philox row row_offset + i and its step counter starts at 0; each
 * utterance's frame records and W·frames GEMMs run with exactly the shapes of that single call
 * (never one GEMM over all utterances: rocBLAS picks its tiling by shape), the per-round
 * interpolation sums in the single call's order, and the list instantiation of the kernel runs the
 * same step code.
 *   mel   [U]  utterance i's [feat_dims][T_i] (device)
 *   aux   [U]  its MelResNet output [res_out_dims][T_i] (device), as wrnn_generate_frames takes it:
 *              the caller runs wrnn_melresnet per utterance, with the shapes of a single call
 *   T     [U]  frame counts, each >= 21
 *   lanes      1..8
 *   noise [U]  utterance i's injected draws [hop·T_i][11] by its own step (device), or noise = NULL
 *              for in-kernel Philox
 *   out   [U]  utterance i's [hop·T_i] fp32 loop output (device)
 * Every argument of every utterance is checked before anything is queued (WRNN_EINVAL: the handle
 * is as before).  WRNN_EUNSUPPORTED under the conditions of wrnn_stream_open: a handle that is
 * not MoL, rows that run on neither the dense one-row XCD kernel (last_path 5) nor the
 * block-sparse rnn-896 one (6), or a cascade wrnn_frame_weights refuses.  Queues its work on
 * `stream` and does not wait for it, except where a workspace must grow (all of them before anything is queued) or the frame weights changed.  One stream per
 * handle, as wrnn_stream_open states; sessions and one-shot calls on the same handle may run
 * before and after it in stream order (the call owns its state records and hand-off tags).  Sets
 * wrnn_info.last_path (5 or 6) and the timing events as wrnn_generate does; kernel aborts surface through
 * wrnn_check. */
int wrnn_list_plan(const int *frames, int U, int lanes, int *lane_of, int *pos_in_lane, int64_t *lane_frames);
int wrnn_generate_list(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                       const int *T, int U, int lanes, const float *const *noise, uint64_t seed, int64_t row_offset,
                       float *const *out, void *stream);

/* ---- Wide lists: a list on up to 128 many-row slots, MoL and RAW (wide-list addition, same ABI) --
 * The one-shot use of the grouped many-row launches of wide sessions: up to 128 SLOTS, 16 per XCD,
 * each running a queue of whole utterances back to back; when an utterance ends its slot goes on
 * with the next of its queue.  The entry a batch of hundreds of sentences calls; the only list form
 * for RAW (9 bits) models.
 *
 * Schedule (wrnn_list_wide_plan; host only, stateless, deterministic).  Assignment: the rule of
 * wrnn_list_plan with `slots` in 1..128 — utterances by decreasing frame count (ties: the lower
 * index first), each to the least loaded slot (ties: the lowest slot); a slot runs its utterances in
 * the order they were assigned.  Launch cuts: a slot's timeline is the concatenation of its
 * utterances' steps (hop per frame).  All rows of a grouped launch run the same number of steps and
 * the kernel takes no per-row mask, so the common timeline is cut at EVERY utterance end on ANY
 * slot, and each piece between two such cuts again into launches of at most
 * wrnn_wide_steps_per_launch(rows, longest timeline in steps, raw) steps (the WRNN_TERMS_MB budget).
 * Lengths are multiples of hop, so no utterance-boundary cut leaves a launch shorter than a frame.
 * The rows of a launch are the slots that still have a step to run, compacted in slot order:
 * launch row r on XCD r % 8, slot r / 8 there; a slot whose queue has ended takes no row.
 *   frames       [U]      frame counts T_i, each >= 21
 *   slots, hop            1..128; steps per frame (>= 1)
 *   raw                   0: MoL budget, 1: RAW budget (the 512 draws share it)
 *   slot_of      [U]      out: the slot of utterance i             (may be NULL, as every output)
 *   pos_in_slot  [U]      out: its place in that slot's queue
 *   slot_frames  [slots]  out: the slot's timeline in frames
 *   launch_first / launch_steps / launch_rows [cap]  out: per launch its first timeline step, its
 *                         steps and its rows (the first `cap` launches)
 * Returns the number of launches; a negative WRNN_EINVAL (message in wrnn_cond_last_error) for
 * U < 1, slots outside 1..128, hop < 1, any T_i < 21, or a timeline past 2^31 − 1 steps.
 *
 * wrnn_generate_list_wide: the arguments of wrnn_generate_list with `slots` (1..128; 0: min(128, U))
 * in place of `lanes`; noise[i] is [hop·T_i][K] by the utterance's own step, K = 11 MoL uniforms or
 * 512 Exp(1) draws for RAW.  It takes a handle wrnn_stream_open_wide would take (MoL or RAW 9 bits,
 * rnn / fc 512, the four-quad grouped form co-resident) and returns WRNN_EUNSUPPORTED with that
 * call's messages otherwise; deepmind handles are refused.  Each utterance's frame-term stores are
 * computed with the launches and shapes of its single many-row call (never one GEMM over several
 * utterances); then the plan's launches run with the sequence of a wide push — per launch one
 * interpolation launch, one draws launch, the hop-area reset, the member counters, one persistent
 * grouped launch.  The row table of the whole call goes up once from pinned memory, every workspace
 * is grown before anything is queued and nothing waits on the stream between launches.  A launch
 * row is its utterance at its own step: stores at base 0, Philox row row_offset + i, a state record
 * that belongs to the utterance and to this call (neither a session's nor a one-shot call's), zero
 * state at the utterance's step 0.  Every argument of every utterance is checked before anything is
 * queued (WRNN_EINVAL: the handle is as before).  Sessions (narrow and wide) and one-shot calls on
 * the same handle may run before and after it in stream order.  Sets wrnn_info.last_path to 7 and
 * the timing events around the loop share (interpolation, draws, resets, persistent launches), as
 * a wide push does.
 *
 * What a wide list promises.
 *   Independence of company: out[i] does not depend on the other utterances, their order, `slots`
 *     or WRNN_TERMS_MB — it is bit-identical to the wide list that holds utterance i alone, called
 *     with row_offset + i (every grouped launch is the four-quad form: rows are independent MFMA
 *     columns).
 *   MoL: within 2·MOL_TOL = 2e-5 of the oracle on the same draws (the wide bound); under Philox within
 *     MOL_TOL of wrnn_generate_frames of utterance i with (seed, row_offset + i).  NOT bit-identical
 *     to wrnn_generate_list or wrnn_generate_frames: another kernel.
 *   RAW: the class labels are the oracle's and wrnn_generate's on the same draws, bit for bit, so
 *     without mu-law expansion every sample before the fade is exact. */
int wrnn_list_wide_plan(const int *frames, int U, int slots, int hop, int raw, int *slot_of, int *pos_in_slot,
                        int64_t *slot_frames, int *launch_first, int *launch_steps, int *launch_rows, int cap);
int wrnn_generate_list_wide(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                            const int *T, int U, int slots, const float *const *noise, uint64_t seed, int64_t row_offset,
                            float *const *out, void *stream);

/* wrnn_postprocess (unbatched) for every utterance of a list in ONE launch: entry i is utterance i's
 * fp32 loop output y [steps] (device), its wave_len (fade_len <= wave_len <= steps) and the offset
 * dst of its float64 waveform in `wave`; the optional mu-law expansion (RAW; mu = n_classes − 1, by
 * wrnn_postprocess's expression) comes before the 20-frame fade-out.  wave[dst .. dst + wave_len)
 * equals wrnn_postprocess(y, 1, steps, 0, 0, mu_law, n_classes, wave_len, fade_len, …) bit for bit
 * (with mu-law on: to the accuracy of pow, rtol 1e-12).  One copy then brings all waveforms to the
 * host.  `entries` [U] lives in device memory; max_wave_len >= every wave_len sizes the grid.
 * WRNN_EINVAL for U outside 1..65535, fade_len < 1 or max_wave_len < fade_len. */
typedef struct {
    const float *y;
    int64_t dst;
    int32_t steps, wave_len;
} wrnn_post_entry;
int wrnn_postprocess_list(const wrnn_post_entry *entries, int U, int max_wave_len, int mu_law, int n_classes,
                          int fade_len, double *wave, void *stream);

/* ---- Folded lists: a list of unequal utterances fold-batched on up to 128 many-row slots (additive,
 * same ABI) ----
 * The reference's default way to vocode (voc_gen_batched: target 11 000, overlap 550) for a list:
 * every utterance is cut into folds of Lf = target + 2·overlap steps (fold_with_overlap), and the
 * folds of ALL utterances are the rows of the grouped many-row launches of wide sessions.  Folds are
 * all the same length, so the common timeline is cut only at fold boundaries (rounds) and by the
 * WRNN_TERMS_MB budget; a long utterance spreads over many slots instead of holding one.
 *
 * Schedule (wrnn_list_folds_plan; host only, stateless, deterministic).  folds[i] is the row count
 * wrnn_cond_shape gives for T_i frames (fold_geometry); folds are numbered utterance-major:
 * first_row[i] = Σ_{j<i} folds[j], F = Σ folds.  Fold g runs in round g / slots as launch row
 * g % slots (XCD r % 8, slot r / 8 there).  A round is Lf steps of the common timeline, cut into
 * launches of at most wrnn_wide_steps_per_launch(rows of the round, Lf, raw) steps.
 *   frames       [U]      frame counts T_i, each >= 21
 *   hop, target, overlap  steps per frame (>= 1); the fold geometry (target >= 1, overlap >= 0)
 *   slots                 1..128; 0: min(128, F)
 *   raw                   0: MoL budget, 1: RAW budget (the 512 draws share it)
 *   folds, first_row [U]  out (may be NULL, as every output)
 *   launch_first / launch_steps / launch_rows [cap]  out: per launch its first step on the common
 *                         timeline (round · Lf + the fold-local step), its steps and its rows
 * Returns the number of launches; a negative WRNN_EINVAL (message in wrnn_cond_last_error) for
 * U < 1, slots outside 0..128, hop < 1, target < 1, overlap < 0, any T_i < 21, hop·T_i < overlap
 * (or an utterance without a fold), or a step or row count past the 32-bit counters.
 *
 * wrnn_generate_list_folds: the arguments of wrnn_generate_list_wide with the fold geometry.
 * out[i] is [folds_i][Lf] fp32 and noise[i], when given, [Lf][folds_i][K] (K = 11 MoL uniforms, 512
 * Exp(1) draws for RAW) — the layouts wrnn_generate_frames takes for utterance i alone.  It takes
 * the handles wrnn_generate_list_wide takes and refuses the others with the same texts.  Each
 * utterance's frame-term stores are computed exactly as the wide list does (never one GEMM over
 * several utterances); the plan's launches run with the sequence of a wide push, a fold-aware
 * table-driven interpolation launch in place of the windowed one: launch step j of a fold row is
 * utterance position p = fold·(target + overlap) + fold-local step; past hop·T_i the terms are
 * W·[0 | 0 | 1] alone (fold_with_overlap's zero tail).  A fold row is Philox row
 * row_offset + first_row[i] + fold at its fold-local step — the keys of
 * wrnn_generate_frames(…, target, overlap, …, row_offset + first_row[i]) of utterance i alone — with
 * a state record of its own that belongs to this call, zero at the fold's step 0.  Every argument of
 * every utterance is checked and every workspace grown before anything is queued.  Sets
 * wrnn_info.last_path to 7 and the timing events as a wide push does.
 *
 * What a folded list promises.
 *   Independence of company: out[i] does not depend on the other utterances, their order, `slots` or
 *     WRNN_TERMS_MB — it is bit-identical to the folded list of utterance i alone with
 *     row_offset + first_row[i].
 *   RAW: out[i] equals the rows of wrnn_generate_frames(target, overlap) of utterance i alone on the
 *     same draws bit for bit (the labels are exact in both).
 *   MoL: after wrnn_postprocess_list_folds within √2 · 2·MOL_TOL = 2.83e-5 of the oracle's batched
 *     generate on the same draws (a sample is the sum of at most two fold samples, each within the
 *     wide bound 2e-5, with cross-fade weights sqrt(½(1 ± t)) whose sum is <= √2); under Philox within
 *     √2 · MOL_TOL of the one-shot batched call.  NOT bit-identical to wrnn_generate_frames: another
 *     instantiation of the kernel. */
int wrnn_list_folds_plan(const int *frames, int U, int hop, int target, int overlap, int slots, int raw, int *folds,
                         int *first_row, int *launch_first, int *launch_steps, int *launch_rows, int cap);
int wrnn_generate_list_folds(wrnn_t *h, const wrnn_upsample_cfg *ucfg, const float *const *mel, const float *const *aux,
                             const int *T, int U, int target, int overlap, int slots, const float *const *noise,
                             uint64_t seed, int64_t row_offset, float *const *out, void *stream);

/* wrnn_postprocess (batched) for every utterance of a folded list in ONE launch: entry i is
 * utterance i's fp32 fold output y [rows][steps] (device), its fold count, its wave_len
 * (fade_len <= wave_len <= rows·(steps − overlap) + overlap) and the offset dst of its float64
 * waveform in `wave`; `steps` (= target + 2·overlap) and `overlap` are call-wide.  Per utterance:
 * the optional mu-law expansion, the fade-in / fade-out of each fold, the sum of at most two folds,
 * the trim to wave_len and the 20-frame fade-out.  wave[dst .. dst + wave_len) equals
 * wrnn_postprocess(y, rows, steps, 1, overlap, mu_law, n_classes, wave_len, fade_len, …) bit for bit
 * (with mu-law on: to the accuracy of pow, rtol 1e-12).  `entries` [U] lives in device memory;
 * max_wave_len >= every wave_len sizes the grid.  WRNN_EINVAL for U outside 1..65535, steps < 1,
 * fade_len < 1, max_wave_len < fade_len, overlap < 0 or steps − 2·overlap < 1. */
typedef struct {
    const float *y;
    int64_t dst;
    int32_t rows, wave_len;
} wrnn_post_fold_entry;
int wrnn_postprocess_list_folds(const wrnn_post_fold_entry *entries, int U, int steps, int overlap, int max_wave_len,
                                int mu_law, int n_classes, int fade_len, double *wave, void *stream);

/* ---- Mel front end: wav in, the normalised mel generate() takes out (additive, same ABI) --------
 * The reference's melspectrogram (utils/dsp.py:41-81) on the device, one launch for any set of
 * frames of any set of signals.  The reference calls librosa; this implements the published
 * definitions, pinned to a float64 restatement of them (tests/melspec_ref.py), not to librosa's
 * output:
 *   yp = reflect-pad(y, n_fft/2) (edge excluded);  T = 1 + len(y)/hop_length frames, frame t =
 *   yp[t·hop : t·hop + n_fft];  window = periodic Hann of win_length, zero-padded to n_fft with
 *   l = (n_fft − win_length)/2 zeros on the left;  |rfft|;  Slaney mel filterbank (fmin .. sr/2,
 *   area-normalised);  clip((20·log10(max(1e-5, S)) − min_level_db) / −min_level_db, 0, 1).
 * Tables are built on the host in float64 and rounded once to float32; the kernel computes in
 * float32, one workgroup per frame, so a frame's value does not depend on the other frames or
 * signals of the launch: the same frame is bit-identical one-shot, chunked and streamed.
 * Taps whose window value is zero (the zero padding, a Hann window's first sample) are never read.
 *
 * WRNN_EUNSUPPORTED (decided without a launch) unless n_fft is a power of two in 256..4096,
 * 1 <= win_length <= n_fft, hop_length >= 1, num_mels <= 128 and 0 <= fmin < sample_rate/2;
 * WRNN_EINVAL for a signal shorter than n_fft/2 + 1 samples (the reflect padding's own limit).
 * Errors leave their text in wrnn_cond_last_error. */
typedef struct {
    int32_t sample_rate;     /* 22050 */
    int32_t n_fft;           /* 2048 */
    int32_t hop_length;      /* 275 */
    int32_t win_length;      /* 1100 */
    int32_t num_mels;        /* 80 */
    float fmin;              /* 40 */
    float min_level_db;      /* -100 */
} wrnn_melspec_cfg;
/* Frames of a signal of n_samples: 1 + n_samples / hop_length (negative: WRNN_E*). */
int64_t wrnn_melspec_frames(const wrnn_melspec_cfg *cfg, int64_t n_samples);
/* The tables (host functions, no GPU): wrnn_melspec_table_floats(cfg) floats, M = n_fft/2 —
 *   [0, 8)            first weighted tap, weighted taps, filterbank weights, then zeros
 *   win   [n_fft]     the zero-padded window
 *   twM   [2·M]       (cos, −sin)(2πn/M), n < M      — the M-point complex FFT of the even/odd packing
 *   twN   [2·(M + 1)] (cos, −sin)(2πk/n_fft), k <= M — its post-twiddle pass
 *   start [num_mels], len [num_mels], off [num_mels]  per band: first non-zero bin, bins, offset in w
 *   w     [Σ len]     the bands' non-zero weights
 * The caller copies them to the device once and passes that pointer as `tables`. */
int wrnn_melspec_table_floats(const wrnn_melspec_cfg *cfg);
int wrnn_melspec_tables(const wrnn_melspec_cfg *cfg, float *host_out);
/* U device signals wav[u] of n[u] samples → U device mels, mel[u][band·ld[u] + t] for t < T_u
 * (ld[u] >= T_u: a caller may write straight into a padded tensor; the padding is not touched).
 * The pointer and length arrays are host arrays.  `scratch` is a device buffer of at least
 * WRNN_MELSPEC_SCRATCH_PER_SIGNAL·U bytes the call fills with its job list; it must stay untouched
 * until the launch has run.  One launch, queued on `stream`.  The job list is copied from pageable
 * host memory, which HIP completes on the host before the call returns: the call may therefore wait
 * for earlier work on `stream` (a caller that pipelines should give the front end a stream of its
 * own and order it with events); the kernel itself runs asynchronously.  The same holds for
 * wrnn_melspec_window and wrnn_melspec_windows. */
#define WRNN_MELSPEC_SCRATCH_PER_SIGNAL 64
int wrnn_melspec(const wrnn_melspec_cfg *cfg, const float *tables, const float *const *wav, const int *n, int U,
                 float *const *mel, const int *ld, void *scratch, void *stream);
/* Frames t0 .. t0 + nt − 1 of a signal of which samples [s0, s0 + ns) are resident at wav_tail
 * (device) → mel[band·ld + (t − t0)].  `total` is the signal's length, or −1 while it is not known:
 * reflection applies at the left edge always and at the right edge only with a known total.
 * WRNN_EINVAL (nothing queued) when a frame reads a sample that is not resident.
 * wrnn_melspec_windows is the same for U signals in one launch (host arrays of U entries). */
int wrnn_melspec_window(const wrnn_melspec_cfg *cfg, const float *tables, const float *wav_tail, int64_t s0, int ns,
                        int64_t total, int t0, int nt, float *mel, int ld, void *scratch, void *stream);
int wrnn_melspec_windows(const wrnn_melspec_cfg *cfg, const float *tables, const float *const *wav_tail, const int64_t *s0,
                         const int *ns, const int64_t *total, const int *t0, const int *nt, int U, float *const *mel,
                         const int *ld, void *scratch, void *stream);
/* Streaming, pure host: with `received` samples in, frames 0 .. *frames_ready − 1 are final, and
 * samples before *keep_from are needed by no later frame (whatever the signal's eventual length).
 * With [wlo, whi) the weighted taps, frame t is final once received >= t·hop + whi − n_fft/2 (for
 * the default geometry t·hop + 550) and frame 0's mirrored samples are in (received >= n_fft/2 − wlo
 * + 1; the same 550 there).  final != 0: `received` is the whole signal, all 1 + received/hop frames
 * are ready (WRNN_EINVAL below n_fft/2 + 1 samples). */
int wrnn_melspec_plan(const wrnn_melspec_cfg *cfg, int64_t received, int final, int64_t *frames_ready,
                      int64_t *keep_from);

/* ---- Tacotron decoder loop (csrc/tacotron_decoder.hip) --------------------------------
 * The reference's Decoder.forward / LSA.forward in eval mode (models/tacotron.py:171-286) and the
 * loop and stop rule of Tacotron.generate (:453-461), for 1..128 rows (one row = one sentence) in
 * ONE persistent launch: prenet on the previous step's last frame, attention GRU cell, LSA (scores =
 * sigmoid(u) / sum sigmoid(u) over the row's own t_enc positions), context, rnn_input, two residual
 * LSTM cells, the r needed rows of mel_proj per mel, and the stop test (every one of the step's
 * n_mels·r values < stop_threshold and step·r > 10; the stopping step's frames are kept).
 * fp32 weights read in place (device pointers to the module's own contiguous tensors, PyTorch
 * layouts), fp32 accumulation; a row's arithmetic does not depend on the other rows or on its slot.
 * Stateless: errors leave their text in wrnn_cond_last_error.  Only the sizes below are taken;
 * anything else is WRNN_EUNSUPPORTED. */
typedef struct {
    int32_t n_mels;        /* 80  */
    int32_t decoder_dims;  /* 256 */
    int32_t lstm_dims;     /* 512 */
    int32_t encoder_dims;  /* 256: channels of encoder_seq (= decoder_dims in the reference) */
    int32_t prenet_fc1;    /* 256 */
    int32_t prenet_fc2;    /* 128 */
    int32_t lsa_filters;   /* 32  */
    int32_t lsa_kernel;    /* 31  */
    int32_t max_r;         /* 20  */
} wrnn_taco_cfg;

/* Device pointers, every one required; shapes as in the reference's state_dict. */
typedef struct {
    const float *prenet_fc1_w, *prenet_fc1_b, *prenet_fc2_w, *prenet_fc2_b;
    const float *attn_rnn_w_ih, *attn_rnn_w_hh, *attn_rnn_b_ih, *attn_rnn_b_hh;
    const float *lsa_conv_w, *lsa_L_w, *lsa_L_b, *lsa_W_w, *lsa_W_b, *lsa_v;
    const float *rnn_input_w, *rnn_input_b;
    const float *res_rnn1_w_ih, *res_rnn1_w_hh, *res_rnn1_b_ih, *res_rnn1_b_hh;
    const float *res_rnn2_w_ih, *res_rnn2_w_hh, *res_rnn2_b_ih, *res_rnn2_b_hh;
    const float *mel_proj_w;
} wrnn_taco_weights;

/* WRNN_OK when the kernel takes these sizes, else WRNN_EUNSUPPORTED with the reason. */
int wrnn_taco_supported(const wrnn_taco_cfg *cfg);
/* The recurrent state is a caller-owned device buffer of rows × wrnn_taco_state_floats(cfg, t_max)
 * floats; a fresh sentence starts from all zeros.  wrnn_taco_state_layout fills the offset (in
 * floats, within a row) of each field, in this order: attn_hidden [decoder_dims], rnn1_hidden,
 * rnn1_cell, rnn2_hidden, rnn2_cell [lstm_dims each], context [decoder_dims], cumulative [t_max],
 * attention [t_max], last frame [n_mels], step (int32: decoder steps done), stopped (int32: 0 / 1).
 * The caller may read and write any of it between calls (tests start from recorded states). */
#define WRNN_TACO_STATE_FIELDS 11
int wrnn_taco_state_floats(const wrnn_taco_cfg *cfg, int t_max);
int wrnn_taco_state_layout(const wrnn_taco_cfg *cfg, int t_max, int32_t *offsets);
int64_t wrnn_taco_scratch_floats(const wrnn_taco_cfg *cfg, int rows);
/* Runs up to n_steps further decoder steps of every row that has not stopped and whose step counter
 * is below step_cap (= ceil(steps / r)); the launch ends early once no such row is left.  Row b reads
 * enc / enc_proj [rows][t_max][encoder_dims] at its first t_enc[b] positions (device int32, each in
 * 1..t_max) and writes step s to mel [rows][step_cap·r][n_mels] (frames s·r .. s·r + r − 1) and attn
 * [rows][step_cap][t_max] (first t_enc[b] entries); a stopped row writes nothing further.  The step
 * counts come back in the state.  Synchronises `stream`.  Every inter-workgroup wait is bounded by
 * timeout_ms (0: 2000): a missed hand-off is WRNN_ETIMEOUT, never a hang.  WRNN_EUNSUPPORTED on a
 * device with fewer than 128 CUs (one workgroup per CU, all co-resident, one owner per row). */
int wrnn_taco_run(const wrnn_taco_cfg *cfg, const wrnn_taco_weights *w, const float *enc, const float *enc_proj,
                  const int32_t *t_enc, int t_max, int rows, int r, float stop_threshold, int step_cap, int n_steps,
                  float *state, float *mel, float *attn, float *scratch, int timeout_ms, void *stream);

/* ---- Tacotron CBHGs for ragged lists (csrc/cbhg.hip) -------------------------------
 * The reference's Encoder (embedding, eval-mode prenet, CBHG) with encoder_proj, and its postnet
 * CBHG with post_proj (models/tacotron.py), for n_seq sentences of n_seq lengths packed end to end
 * on the time axis: position p of the packed axis is row p of every [positions][channels] buffer,
 * and sentence i owns positions offsets[i] .. offsets[i + 1] − 1.  Stages are separate launches on
 * the caller's stream; no workgroup waits for another.  fp32 weights, fp32 accumulation; a
 * sentence's values do not depend on the other sentences, on its slot or on n_seq, bit for bit.
 * Stateless: errors leave their text in wrnn_cond_last_error.  Two size sets are taken (the
 * reference's hparams); anything else is WRNN_EUNSUPPORTED. */
typedef struct {
    int32_t K;            /* bank kernels 1..K: 16 (encoder) / 8 (postnet) */
    int32_t in_channels;  /* 128 / 80 */
    int32_t channels;     /* 128 */
    int32_t proj1;        /* 128 / 256 */
    int32_t proj2;        /* 128 / 80 (= in_channels: the residual) */
    int32_t pre_highway;  /* 0 / 1: the bias-free proj2 → channels linear */
    int32_t highways;     /* 4 */
    int32_t front;        /* 1: the input is int32 ids (embedding, prenet fc1 → ReLU → fc2 → ReLU) / 0: float rows */
    int32_t embed_dims;   /* 256 / 0 */
    int32_t num_chars;    /* rows of the embedding (any >= 1) / 0 */
    int32_t prenet_fc1;   /* 256 / 0 */
    int32_t tail_out;     /* outputs of the bias-free tail over the GRU output: 256 (encoder_proj) / fft_bins 80 (post_proj) */
} wrnn_cbhg_cfg;

#define WRNN_CBHG_MAX_K 16
#define WRNN_CBHG_HIGHWAYS 4
/* Device pointers to the module's own contiguous fp32 tensors, PyTorch layouts (conv [out][in][k],
 * linear [out][in]); read by every call, nothing is cached.  Entries beyond K, and the front's /
 * pre_highway's where the cfg has none, are ignored. */
typedef struct {
    const float *embedding, *prenet_fc1_w, *prenet_fc1_b, *prenet_fc2_w, *prenet_fc2_b;
    const float *bank_w[WRNN_CBHG_MAX_K], *bank_bn_w[WRNN_CBHG_MAX_K], *bank_bn_b[WRNN_CBHG_MAX_K];
    const float *bank_bn_mean[WRNN_CBHG_MAX_K], *bank_bn_var[WRNN_CBHG_MAX_K];
    const float *proj1_w, *proj1_bn_w, *proj1_bn_b, *proj1_bn_mean, *proj1_bn_var;
    const float *proj2_w, *proj2_bn_w, *proj2_bn_b, *proj2_bn_mean, *proj2_bn_var;
    const float *pre_highway_w;
    const float *hw_w1[WRNN_CBHG_HIGHWAYS], *hw_b1[WRNN_CBHG_HIGHWAYS], *hw_w2[WRNN_CBHG_HIGHWAYS], *hw_b2[WRNN_CBHG_HIGHWAYS];
    const float *rnn_w_ih, *rnn_w_hh, *rnn_b_ih, *rnn_b_hh;          /* forward direction, gates r z n */
    const float *rnn_w_ih_r, *rnn_w_hh_r, *rnn_b_ih_r, *rnn_b_hh_r;  /* reverse direction */
    const float *tail_w;
} wrnn_cbhg_weights;

/* WRNN_OK when the kernels take these sizes, else WRNN_EUNSUPPORTED with the reason. */
int wrnn_cbhg_supported(const wrnn_cbhg_cfg *cfg);
/* Bytes of device scratch a run over `positions` packed positions needs (any n_seq <= positions). */
int64_t wrnn_cbhg_scratch_bytes(const wrnn_cbhg_cfg *cfg, int64_t positions);
/* Offsets, in floats from the scratch's start, of the stage buffers that are intact after a run, in
 * this order (−1: the cfg has no such stage): front output [positions][in_channels], bank
 * [positions][K·channels] (ReLU and BatchNorm applied), pooled bank (same shape), conv_project1
 * output [positions][proj1], highway-stack input before pre_highway (conv_project2 + residual)
 * [positions][proj2], highway input [positions][channels] (the same buffer without pre_highway),
 * highway output [positions][channels], GRU input terms [positions][6·channels], GRU output
 * [positions][2·channels]. */
#define WRNN_CBHG_STAGES 9
int wrnn_cbhg_scratch_layout(const wrnn_cbhg_cfg *cfg, int64_t positions, int64_t *offsets);
/* One pass over n_seq sentences.  `offsets` is a HOST array of n_seq + 1 entries, offsets[0] = 0,
 * strictly increasing (every sentence has a position); `input` is device memory: int32 ids
 * [positions] with the front, else float [positions][in_channels].  out_rnn [positions][2·channels]
 * (may be NULL) and out_proj [positions][tail_out] are device buffers.  Everything is checked
 * before anything is queued (WRNN_EINVAL): null or misaligned (16 bytes) pointers, n_seq < 1, the
 * offsets, scratch_bytes below wrnn_cbhg_scratch_bytes, an id outside the embedding (the ids are
 * read back for that).  Synchronises `stream` once before the stages are queued (the position
 * tables' upload) and not after them. */
int wrnn_cbhg_run(const wrnn_cbhg_cfg *cfg, const wrnn_cbhg_weights *w, const void *input, const int32_t *offsets,
                  int n_seq, float *out_rnn, float *out_proj, void *scratch, int64_t scratch_bytes, void *stream);

/* Message of the last failed stateless call on this thread. */
const char *wrnn_cond_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* WAVERNN_AMD_H */
