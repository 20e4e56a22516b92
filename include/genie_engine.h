/*
 * genie_engine.h -- C ABI of the MI355X GPT-SoVITS engine (libgenie_engine.so).
 *
 * Drop-in replacement for the onnxruntime InferenceSession objects that Genie
 * holds per character in `GSVModel` (reference: src/genie_tts/ModelManager.py:48-56)
 * and calls from `GENIE.tts` / `GENIE.t2s_cpu` (src/genie_tts/Core/Inference.py:16-109).
 *
 *   reference call                                   replaced by
 *   ------------------------------------------------ ------------------------------------
 *   load_session_with_fp16_conversion (ModelManager.py:59-114)
 *                                                    gsv_engine_create + gsv_set_weight
 *                                                    + gsv_finalize_weights
 *   encoder.run            (Inference.py:76-85)      gsv_t2s_encode
 *   first_stage_decoder.run(Inference.py:88-90)      gsv_t2s_prefill
 *   stage_decoder.run      (Inference.py:102)        gsv_t2s_decode_steps (k steps)
 *   the 500-step loop + trim (Inference.py:95-109)   gsv_t2s_generate (the whole loop as ONE persistent
 *                                                    kernel launch; per-step hipGraphs only as a fallback)
 *   vocoder.run            (Inference.py:47-60)      gsv_vits_decode
 *   prompt_encoder.run     (ReferenceAudio.py:73)    gsv_prompt_encode
 *   vocoder.run's refer branch (Inference.py:50, V2)  gsv_ref_encode (once per reference)
 *   aux_ref_audio_paths    (GPT-SoVITS: the mean of the clips' ge in SynthesizerTrn.decode)
 *                                                    gsv_ge_mix (+ gsv_ge_project on V2ProPlus)
 *   cn_hubert.run          (ReferenceAudio.py:50-52) gsv_hubert
 *   roberta_model.run      (GetPhonesAndBert.py:73)  gsv_roberta (gsv_roberta_batch: many sentences)
 *   per-sentence tts loop  (TTSPlayer.py:56-107)     gsv_t2s_prefetch, gsv_t2s_generate_start /
 *                                                    _finish, gsv_vits_decode_async / gsv_vits_wait
 *                                                    (option "vocoder_cus")
 *   stop_event.set()/.clear() (Inference.py:13-14,96-97) gsv_request_stop
 *
 * Conventions
 *   - All functions return 0 on success, a negative GSV_E* code on failure;
 *     gsv_last_error() returns a thread-local message for the last failure.
 *   - Weights are engine-owned device memory.  Every other pointer argument
 *     marked (device) is a caller-owned device buffer (e.g. a torch tensor's
 *     data_ptr()); (host) arguments are read before the call returns.
 *   - `stream` is the caller's hipStream_t passed as void* (NULL = the HIP null
 *     stream).  The engine runs on its own stream, ordered after `stream` on
 *     entry and before it on exit by events: results are stream-ordered for
 *     the caller.
 *     Calls on one engine are serialised by the caller (one engine per GPU
 *     process, as the reference serialises on its single TTS worker thread,
 *     Core/TTSPlayer.py:55).
 *   - Integer ids are int64 (the graphs' dtype); audio/features fp32.
 */
#ifndef GENIE_ENGINE_H
#define GENIE_ENGINE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSV_OK 0
#define GSV_E_ARG -1
#define GSV_E_HIP -2
#define GSV_E_STATE -3
#define GSV_E_WEIGHT -4
#define GSV_E_CAPACITY -5
#define GSV_E_STOPPED -6   /* the generate was abandoned by gsv_request_stop (the reference returns None) */

typedef struct gsv_engine gsv_engine;

/* dtype codes for gsv_set_weight */
#define GSV_F32 0
#define GSV_F16 1

/* Model families (ModelManager.py:287-293: prompt encoder present => V2ProPlus). */
#define GSV_V2 0
#define GSV_V2PP 1

const char* gsv_last_error(void);
const char* gsv_version(void);

/* Create an engine on HIP device `device` for model family `version`. */
int gsv_engine_create(int device, int version, gsv_engine** out);
int gsv_engine_destroy(gsv_engine* eng);

/* Stage one weight tensor (host memory, any of GSV_F32/GSV_F16) by its graph
 * initializer name (e.g. "transformer_encoder.layers.0.linear1.weight",
 * "vq_model.dec.ups.0.weight_v").  Copied before return. */
int gsv_set_weight(gsv_engine* eng, const char* name, const void* host, int dtype,
                   const int64_t* dims, int ndim);

/* Fold weight norm (w = v/||v|| * g), convert, upload; must follow the last
 * gsv_set_weight.  Missing tensors are an error (GSV_E_WEIGHT).  No weight is ever
 * rounded silently: the T2S / VITS / prompt-encoder paths take fp16 weights (the
 * Genie fp16 bins, ModelManager.py:59-114) and refuse a tensor that is not
 * fp16-exact (GSV_E_WEIGHT naming it); RoBERTa and CN-HuBERT keep fp32 values
 * (RoBERTa.onnx is loaded as fp32, ModelManager.py:139-142) as fp16 hi + lo planes
 * (counter "w16_split_tensors"). */
int gsv_finalize_weights(gsv_engine* eng);

/* Host-only check used by those loaders: 1 if all n values are exactly fp16 numbers,
 * else 0 with *first_bad = the first index that is not (-1 when all are).  Needs no
 * device. */
int gsv_f16_exact(const float* values, int64_t n, int64_t* first_bad);

/* Reserve decode capacity: up to `max_batch` sequences of up to `max_tokens`
 * positions (x + prompts + generated) each.  Allocates the KV cache. */
int gsv_reserve(gsv_engine* eng, int max_batch, int max_tokens);

/* ---------------------------------------------------------------- T2S ---- */
/* One utterance of a batch.  All pointers (device). */
typedef struct {
    const int64_t* ref_seq;   int32_t n_ref;    /* phonemes of the reference text  */
    const int64_t* text_seq;  int32_t n_text;   /* phonemes of the target text     */
    const float*   ref_bert;                    /* [n_ref, 1024]  or NULL = zeros  */
    const float*   text_bert;                   /* [n_text, 1024] or NULL = zeros  */
    const float*   ssl;       int32_t n_ssl;    /* ssl_content [768, n_ssl]        */
    int32_t force_steps;                        /* >0: this utterance ignores EOS and runs
                                                   exactly this many loop steps (overrides
                                                   gsv_sampler.force_steps; benchmarks and
                                                   ragged-batch tests); 0: the sampler's rule */
} gsv_utt;

/* Sampler (reference constants: t2s_stage_decoder_fp32.onnx#1780-1801).
 *
 * Nucleus sampling (`top_p`, GPT-SoVITS logits_to_probs; the ONNX graphs were exported
 * with top_p = 1, so they never show it).  All values float32, per sequence and step:
 *   1. the repetition penalty over the history tokens gives l[0..1025);
 *   2. only when top_p < 1: p = softmax(l) (before the temperature); the tokens are
 *      ordered by l descending, equal l by ascending index; S_i is the inclusive
 *      cumulative sum of p in that order; token i is removed (l_i := -inf) iff
 *      S_i > top_p and i is not first in the order.  The first token always survives,
 *      the token that crosses top_p is removed (the mask is not shifted);
 *   3. l / temperature, the top-k threshold, softmax and argmax(p / q) as without it
 *      (fewer survivors than top_k: every survivor stays).
 *   0 < top_p <= 1, or 0 = unset = 1 (a zero-initialised gsv_sampler behaves as
 *   before); NaN, negative or > 1: GSV_E_ARG.  Greedy decoding ignores top_p (the
 *   maximum always survives); the first-stage (prefill) sampler applies it too; the
 *   stop rule (argmax of the raw logits) is unchanged.  With top_p unset or 1 every
 *   path does exactly the work it did without the field, and the same tokens. */
typedef struct {
    int32_t top_k;               /* 15 (1..64) */
    float   temperature;         /* 1.0 */
    float   repetition_penalty;  /* 1.35 */
    int32_t greedy;              /* 1: RandomNormalLike := 1 (argmax of penalised logits) */
    uint64_t seed;               /* Philox key for N(0,1) when !greedy */
    int32_t max_steps;           /* 500 (Inference.py:95) */
    int32_t force_steps;         /* >0: ignore EOS and run exactly this many loop steps */
    float   top_p;               /* nucleus cut in (0, 1]; 0 == 1.0 == off (see above) */
} gsv_sampler;

/* Encoder (t2s_encoder_fp32.onnx) for one utterance:
 * x (device, [n_ref+n_text, 512] f32), prompts (device, [n_ssl/2] i64). */
int gsv_t2s_encode(gsv_engine* eng, const gsv_utt* u, float* x, int64_t* prompts, void* stream);

/* Full T2S of a batch: encoder, prefill (one packed pass over the batch), the decode
 * loop on the device, and the reference's token trim + EOS filter
 * (Inference.py:41-44,108-109).  The loop is one persistent kernel launch: B = 1 on
 * k_decode_persist1, B = 2..64 on its multi-sequence form k_decode_persist1m (each
 * layer's workgroups run the live sequences one after another); B > 64, an activation
 * beyond the fp16 range, or a launch whose grid could not be co-resident (a hand-off
 * timeout) re-run on replayed per-step hipGraphs.  out_tokens (host)
 * [batch][out_stride] i64, out_len (host) [batch].  Returns the trimmed semantic tokens
 * per utterance; GSV_E_STOPPED when gsv_request_stop interrupted it. */
int gsv_t2s_generate(gsv_engine* eng, int batch, const gsv_utt* utts, const gsv_sampler* s,
                     int64_t* out_tokens, int32_t out_stride, int32_t* out_len, void* stream);

/* gsv_t2s_generate with one sampler per sequence: samplers[b] is sequence b's, in one launch.
 * The decode kernels read a device table of batch entries (top_k, temperature,
 * repetition_penalty, top_p, greedy, seed and the stream word) at every sampler site: the
 * prefill's first-stage sampler, the persistent kernels, the per-step graphs and a re-run on them.
 *
 * The stream word: the Philox counter of the sampling noise is (token index, loop step,
 * stream, 0x51) under the key `seed`.  gsv_t2s_generate fills `stream` with the batch slot, so a
 * sampled sentence in slot i > 0 draws other noise than alone in slot 0.  Here streams[b] is
 * that word for sequence b (>= 0; NULL: streams[b] = b, the numbering of gsv_t2s_generate).
 * A sequence with streams[b] = 0 draws what a batch-1 generate with its sampler draws, whatever
 * slot it is in and whatever else is in the batch.
 *
 * Every entry is checked as gsv_t2s_generate checks its sampler; a bad one gives GSV_E_ARG and
 * the message names its index.  max_steps is launch-wide: it must be equal in all entries
 * (GSV_E_ARG otherwise).  An entry's force_steps is that sequence's forced length unless its
 * gsv_utt.force_steps is set, which wins, as in gsv_t2s_generate.
 *
 * Greedy: the fused-argmax step end is a launch-wide mode.  It runs only when every entry is
 * greedy with one repetition_penalty and one temperature; then the launch is exactly
 * gsv_t2s_generate's.  Otherwise the launch runs the sampler workgroups and a greedy entry takes
 * the sampler's own greedy branch: the argmax of penalised / temperature, where the fused step
 * end takes the argmax of penalised.  These are the same tokens at temperature 1; at another
 * temperature the division could break a tie of two nearly equal logits differently.
 *
 * With equal entries and streams NULL the tokens are gsv_t2s_generate's, bit for bit.  A
 * prefetched utterance (gsv_t2s_prefetch) is not taken by this call. */
int gsv_t2s_generate_each(gsv_engine* eng, int batch, const gsv_utt* utts,
                          const gsv_sampler* samplers /* [batch] */,
                          const int32_t* streams      /* [batch], or NULL: streams[b] = b */,
                          int64_t* out_tokens, int32_t out_stride, int32_t* out_len, void* stream);

/* Parity/session entry points mirroring the reference graphs one call at a time.
 * prefill: x (device [L,512]), prompts (device [P]) -> writes slot `seq` of the
 *   engine KV cache, y (device i64 [P+1]), logits (device f32 [1025], may be NULL).
 * decode_steps: runs `steps` stage-decoder steps on slot `seq`, appending to y
 *   (device i64, capacity >= P+1+steps); stop (device u8 [steps]);
 *   logits (device [steps][1025] or NULL). */
int gsv_t2s_prefill(gsv_engine* eng, int seq, const float* x, int32_t n_x, const int64_t* prompts,
                    int32_t n_prompts, const gsv_sampler* s, int64_t* y, float* logits, void* stream);
int gsv_t2s_decode_steps(gsv_engine* eng, int seq, int steps, const gsv_sampler* s, int64_t* y,
                         uint8_t* stop, float* logits, void* stream);
/* Copy the KV cache of slot `seq`, layer `layer` as [n,512] k and v (device). */
int gsv_t2s_read_kv(gsv_engine* eng, int seq, int layer, float* k, float* v, int32_t* n, void* stream);

/* --------------------------------------------------------------- VITS ---- */
/* vits_fp32.onnx.  text_seq (device i64 [n_text]), sem (device i64 [n_sem]).
 * V2: ref_audio (device f32 [n_audio] at 32 kHz), ge/ge_adv NULL; or ref_audio NULL and
 *     ge (device [512]) from gsv_ref_encode of that audio (identical output).
 * V2ProPlus: ge (device [1024]), ge_adv (device [512]), ref_audio NULL.
 * eps: (device [192, 2*n_sem]) noise for z_p, or NULL => zeros.
 * audio (device f32 [640*2*n_sem]).  Speech rate 1; gsv_vits_decode_item takes a rate. */
int gsv_vits_decode(gsv_engine* eng, const int64_t* text_seq, int32_t n_text,
                    const int64_t* sem, int32_t n_sem, const float* ref_audio, int32_t n_audio,
                    const float* ge, const float* ge_adv, const float* eps, float noise_scale,
                    float* audio, void* stream);

/* Several vocoder calls at once (the same graph per utterance, vits_fp32.onnx).  Option
 * "seg_vocoder" 1 (default): each utterance's text/flow part runs on the engine's lanes
 * (internal streams, own workspaces), then the HiFi-GAN generator runs ONCE over all of
 * them laid out back to back along time with zero gaps between utterances (every conv
 * treats a gap as the zero padding a single call sees), so its ~400 launches serve the
 * whole batch; each utterance matches its own gsv_vits_decode to fp32 rounding (the
 * batch's larger tiles order the reductions differently).  With option "seg_front" 1
 * (default) the text/flow part is packed the same way (one pass, attention within each
 * utterance) whenever every item carries ge (+ ge_adv) and noise_mode 0 or 2; otherwise
 * it runs per item on the lanes.  seg_vocoder 0: whole utterances on the lanes,
 * bit-identical to single calls.  Results are stream-ordered for the caller like
 * gsv_vits_decode.
 * Noise for z_p (vits(v2)#6490 RandomNormalLike x noise_scale):
 *   noise_mode 0: zeros; 1: eps (device [192, 2*n_sem]); 2: the engine's Philox
 *   N(0,1) stream keyed by noise_seed (counter = element index; Box-Muller).
 *
 * Speech rate (`speed`, GPT-SoVITS TextEncoder.forward's argument; the ONNX graphs were
 * exported with it fixed at 1): the 192-channel latent is resampled linearly along time
 * between enc_p.encoder2 and enc_p.proj, from T = 2*n_sem to T' frames, and proj, the noise,
 * the reverse flows and the generator run at T'.  Pitch is unchanged; the audio is
 * 640 * T' samples.
 *   T' = gsv_vits_frames(n_sem, speed): T when speed == 0 or 1 (a zero-initialised item
 *   means "as before"), else (int)((double)T / (double)speed) + 1 -- the float32 speed
 *   widened to double, so callers take T' from gsv_vits_frames and never recompute it
 *   (n_sem = 11: the double 1.1 gives 21, the float32 1.1 gives 20).  Valid: finite,
 *   0.25 <= speed <= 4 (else GSV_E_ARG; gsv_vits_frames returns GSV_E_ARG);
 *   T' > 4096 is GSV_E_CAPACITY (the generator workspace grows with T').
 *   Resample (ATen's align_corners = False formula in float32, every multiply and add rounded
 *   on its own): scale = (float)T / (float)T'; src = max(scale * (j + 0.5f) - 0.5f, 0);
 *   i0 = min((int)src, T-1); i1 = i0 + (i0 < T-1); l1 = src - i0; l0 = 1 - l1;
 *   out[c][j] = l0 * y[c][i0] + l1 * y[c][i1].
 *   eps is [192, T'] then, and the Philox counter is the element index over 192 * T'.
 * In a batch every item has its own speed.  The segmented generator pass lays the
 * utterances out by T'_i; the packed front ("seg_front") is used only when every item's
 * T' equals its T, otherwise the fronts run per item on the lanes.
 *
 * Output format (`out_rate`, `out_format`, `out`; the reference delivers 16-bit PCM chunks at
 * 32 kHz, and a caller who needs another rate resamples on the host).  The engine's audio is
 * 32 kHz float32; the output stage converts it on the GPU in one launch.
 *   Rates: out_rate in {8000, 16000, 22050, 24000, 32000, 44100, 48000}; 0 means 32000; anything
 *   else is GSV_E_ARG.  g = gcd(32000, out_rate), up = out_rate / g, down = 32000 / g
 *   (1/4, 1/2, 441/640, 3/4, 1/1, 441/320, 3/2).
 *   Length: n_out = gsv_audio_samples(n_in, out_rate) = ceil(n_in * up / down) in integers, the
 *   one place it is computed.
 *   Filter (scipy.signal.resample_poly's default, restated): m = max(up, down), half = 10 m,
 *   2 half + 1 taps, h[i] = (1/m) sinc((i - half) / m) I0(5 sqrt(1 - ((i - half) / half)^2)) / I0(5),
 *   sinc(t) = sin(pi t) / (pi t), I0 by its power series, all in double; h is normalised to sum 1,
 *   multiplied by up and rounded once to float32.
 *   Resample: y[k] = sum_n h[k * down + half - n * up] * x[n] over 0 <= n < n_in with the h index
 *   inside [0, 2 half]: zeros outside the signal, no edge extension.  Each y[k] is ONE float32
 *   chain over ascending n (acc = 0; acc = fmaf(h, x[n], acc)); terms whose coefficient or sample
 *   is a padding zero may be included.  No split sums, no order that depends on a tile: every
 *   entry point gives the same bits for the same input.  out_rate 32000 is a plain copy.
 *   Format: out_format 0 is float32 y; 1 is signed 16-bit,
 *   (int16) trunc(min(max(y * 32767.0f, -32768.0f), 32767.0f)) -- the reference's
 *   (x * 32767).astype(int16) with saturation (the vocoder's tanh stays within 1; the resampled
 *   signal can overshoot).  Another out_format is GSV_E_ARG.
 * In an item: `audio` (32 kHz float32) is still required and written; when `out` is non-NULL the
 * stage also writes out[gsv_audio_samples(640 * gsv_vits_frames(n_sem, speed), out_rate)] (float32
 * or int16 elements) from the item's final audio -- after an fp16-range re-run, from the re-run's.
 * A zero-initialised tail (out NULL) means "as before", and the two fields are then ignored; with
 * `out`, a bad rate or format is GSV_E_ARG before any launch.  Every vocoder entry point that
 * takes items honours the fields; a batch is one stage launch, each item its own rate and
 * format; under gsv_vits_decode_async the stage runs on the vocoder's stream. */
typedef struct {
    const int64_t* text_seq; int32_t n_text;   /* device */
    const int64_t* sem;      int32_t n_sem;    /* device */
    const float* ref_audio;  int32_t n_audio;  /* V2: device 32 kHz audio (or NULL with ge), else NULL */
    const float* ge;         const float* ge_adv;   /* V2ProPlus: device [1024], [512];
                                                       V2: optional ge [512] of gsv_ref_encode */
    const float* eps;                          /* noise_mode 1 */
    uint64_t noise_seed;                       /* noise_mode 2 */
    int32_t noise_mode;
    float* audio;                              /* device [640 * gsv_vits_frames(n_sem, speed)] */
    float speed;                               /* speech rate, 0 == 1.0 (see above) */
    int32_t out_rate;                          /* output stage: sample rate of `out`, 0 == 32000 */
    int32_t out_format;                        /* 0: float32, 1: int16 */
    void* out;                                 /* device [gsv_audio_samples(..)] or NULL: no stage */
} gsv_vits_item;
int gsv_vits_frames(int32_t n_sem, float speed);
/* Samples of n_in 32 kHz samples at out_rate (see above); GSV_E_ARG for an unsupported rate or a
 * negative n_in.  Pure: needs no device. */
int gsv_audio_samples(int32_t n_in, int32_t out_rate);
/* The output stage alone: audio_32k (device f32 [n_in]) -> out (device, float32 or int16
 * [gsv_audio_samples(n_in, out_rate)]), stream-ordered like every other call. */
int gsv_audio_convert(gsv_engine* eng, const float* audio_32k, int32_t n_in, int32_t out_rate,
                      int32_t out_format, void* out, void* stream);
/* One utterance, synchronously, as gsv_vits_decode but described by an item (so with its
 * speed and noise_mode 2).  Bit-identical to gsv_vits_decode for speed 0 or 1 and
 * noise_mode 0 or 1. */
int gsv_vits_decode_item(gsv_engine* eng, const gsv_vits_item* item, float noise_scale, void* stream);
int gsv_vits_decode_batch(gsv_engine* eng, int32_t n, const gsv_vits_item* items, float noise_scale,
                          void* stream);

/* The same batch, overlapped with the T2S of the next batch (a server batching the
 * next sentence of every pending request; each sentence a full Inference.tts,
 * Core/Inference.py:16-61).  gsv_vits_decode_batch_async forks the batch over the
 * vocoder lanes (ordered after `stream`) and returns while lane threads may still be
 * issuing; the engine stream stays free, so a gsv_t2s_generate issued next runs
 * beside it.  Items and their buffers must stay valid until gsv_vits_batch_wait,
 * which joins the lanes, re-runs fp16-range overflows on the f32 path and orders
 * `stream` (may be NULL) after the batch.  Any other vocoder call finishes it first.
 * Audio is identical to gsv_vits_decode_batch's. */
int gsv_vits_decode_batch_async(gsv_engine* eng, int32_t n, const gsv_vits_item* items, float noise_scale,
                                void* stream);
int gsv_vits_batch_wait(gsv_engine* eng, void* stream);

/* Overlapped vocoder for a stream of sentences (the reference synthesises them one
 * after the other: TTSPlayer._tts_worker_loop, Core/TTSPlayer.py:56-107, each
 * sentence a full Inference.tts, Core/Inference.py:16).  After
 * gsv_set_option(eng, "vocoder_cus", K) the engine stream runs on n_cu - K CUs and
 * the vocoder on the other K, so sentence i's vocoder overlaps sentence i+1's T2S.
 * gsv_vits_decode_async starts one vocoder call (ordered after `stream`) and returns
 * without waiting; the item's buffers must stay valid until gsv_vits_wait, which
 * finishes it (fp16-range overflow -> the f32 re-run, as gsv_vits_decode) and orders
 * `stream` (may be NULL) after it.  One call in flight: a second async call, any
 * other vocoder call or gsv_prompt_encode finishes the pending one first. */
int gsv_vits_decode_async(gsv_engine* eng, const gsv_vits_item* item, float noise_scale, void* stream);
int gsv_vits_wait(gsv_engine* eng, void* stream);

/* Loudness normalisation (the reference and GPT-SoVITS only clip, so voices differ by several dB;
 * a caller who wants one level runs a normaliser over the PCM on the host).  The engine measures
 * an item's final 32 kHz float32 audio by ITU-R BS.1770-4 (mono, channel weight 1) and the output
 * stage applies the gain to a target under a sample-peak ceiling (EBU R 128), all on the GPU.
 *   K-weighting: two biquads at 32 kHz.  gsv_loudness_coeffs gives them for any rate, in double:
 *   shelf  f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196, K = tan(pi f0 / fs),
 *          Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2,
 *          b = [(Vh + Vb K/Q + K^2)/a0, 2 (K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *          a = [1, 2 (K^2 - 1)/a0, (1 - K/Q + K^2)/a0];
 *   high-pass f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1],
 *          a = [1, 2 (K^2 - 1)/(1 + K/Q + K^2), (1 - K/Q + K^2)/(1 + K/Q + K^2)]
 *   (at 48000 the standard's table).  The engine rounds them to float32 and runs the recurrence
 *   and the squares in float32 over the whole signal: the impulse response is not truncated.
 *   Hop energies: e_j = sum of the squared filtered samples over [3200 j, 3200 (j + 1)) (100 ms).
 *   A gating block is 4 hops, z_j = (e_j + .. + e_{j+3}) / 12800, j = 0 .. n/3200 - 4 (400 ms,
 *   75 % overlap); samples after the last full block are not measured.
 *   Gating: l_j = -0.691 + 10 log10 z_j; G = -0.691 + 10 log10(mean z over l_j > -70) - 10; the
 *   loudness is -0.691 + 10 log10(mean z over l_j > -70 and l_j > G), blocks_kept their count.
 *   n < 12800: one ungated block over all n samples, its loudness reported; it counts as kept
 *   when above -70.  No block kept, or n == 0: gain 1, blocks_kept 0 (and, with full blocks or
 *   n == 0, loudness -inf).
 *   peak = max |audio|.  gain = min(10^((target - loudness) / 20), ceiling / peak) (the first term
 *   when peak == 0), from the float32 loudness and peak, written as float32 on the device: no host
 *   round trip lies between the measurement and the stage that applies it.
 *   stats = {loudness_lufs, peak, gain, blocks_kept} (device float[4]).  Every sum has one order
 *   whatever the launch: an item gives the same bits alone, in a batch and on the vocoder stream.
 *   Applying: y = chain * gain, one rounded float32 multiply after the output stage's fma chain (or
 *   after the copy at 32000), then the conversion above.  `audio` stays unnormalised.
 * gsv_loudness rides beside an item (gsv_vits_item cannot grow): target LUFS, 0 == off for this
 * item, valid -50 <= target <= -5 else GSV_E_ARG; peak: linear ceiling in (0, 1], 0 == 10^(-1/20)
 * (-1 dBFS, EBU R 128); stats: device float[4] or NULL.  An item with target != 0 needs `out`
 * (out_rate 0 / out_format 0: a normalised 32 kHz float32 copy), else GSV_E_ARG before any launch;
 * the signal is at most 640 * 4096 samples. */
typedef struct { float target; float peak; float* stats; } gsv_loudness;
/* out = shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2 at `rate`.  Pure: needs no device. */
int gsv_loudness_coeffs(int32_t rate, double* out /* [10] */);
/* The `_norm` twins of the entries that take items: norm is [n] (one per item; NULL: the plain
 * call, which forwards here: one set of checks, the same launches).  A batch is one measurement pass
 * plus one stage launch per 256 items; after an fp16-range re-run the re-run's audio is measured;
 * under gsv_vits_decode_async_norm both run on the vocoder's stream.  norm is copied: it need
 * not outlive the call (the stats buffers must, until the wait). */
int gsv_vits_decode_item_norm(gsv_engine* eng, const gsv_vits_item* item, const gsv_loudness* norm,
                              float noise_scale, void* stream);
int gsv_vits_decode_batch_norm(gsv_engine* eng, int32_t n, const gsv_vits_item* items, const gsv_loudness* norm,
                               float noise_scale, void* stream);
int gsv_vits_decode_batch_async_norm(gsv_engine* eng, int32_t n, const gsv_vits_item* items,
                                     const gsv_loudness* norm, float noise_scale, void* stream);
int gsv_vits_decode_async_norm(gsv_engine* eng, const gsv_vits_item* item, const gsv_loudness* norm,
                               float noise_scale, void* stream);
/* The measurement alone: audio_32k (device f32 [n], n <= 640 * 4096) -> stats (device float[4],
 * gain 1), stream-ordered. */
int gsv_audio_loudness(gsv_engine* eng, const float* audio_32k, int32_t n, float* stats, void* stream);
/* Measure and convert: gsv_audio_convert with the gain to `target` (as gsv_loudness: -50 .. -5;
 * peak 0 == -1 dBFS) applied; stats device float[4] or NULL.  Stream-ordered. */
int gsv_audio_normalize(gsv_engine* eng, const float* audio_32k, int32_t n_in, float target, float peak,
                        int32_t out_rate, int32_t out_format, void* out, float* stats, void* stream);
/* Debug: the hop energies e[n / 3200] of audio (device f32 [n]) alone, so the filter and its carry
 * can be tested apart from the gate. */
int gsv_debug_loudness_hops(gsv_engine* eng, const float* audio, int32_t n, float* e, void* stream);

/* Sentence join: the pause behind a sentence and the trim of its edge silence (GPT-SoVITS appends
 * `fragment_interval` seconds of zeros to every fragment; the sentences of a stream are otherwise
 * butt-joined, each with the uneven lead-in its vocoder pass produced).  The engine finds where an
 * item's speech begins and ends on the GPU, and the output stage converts only that span and
 * appends the pause: no host round trip lies between the measurement and the conversion.
 *   Frames: the item's final 32 kHz float32 audio x[0..n) is cut into frames of 320 samples
 *   (10 ms); the last may be partial, with c samples (else c = 320).  Frame f is active when
 *   sum x[i]^2 > T * c, the squares and the sum taken in double (a float32 squared is exact in
 *   double), T = 10^(trim / 10) computed once on the host in double from the float32 trim widened
 *   to double.
 *   Span: f0 and f1 the first and last active frames; begin = max(0, 320 f0 - 640),
 *   end = min(n, 320 (f1 + 1) + 640): a guard of GSV_JOIN_GUARD = 640 samples (20 ms) on either
 *   side.  No active frame, or n == 0: begin = end = 0, and the sentence is its pause alone.
 *   Without a trim the span is [0, n).
 *   Output: n_speech = gsv_audio_samples(end - begin, out_rate);
 *   pause_n = gsv_join_pause_samples(out_rate, pause) = (int)((double)out_rate * (double)pause), the
 *   float32 pause widened to double (out_rate 0 is 32000): callers take it from that function and
 *   never recompute it.  out[0 .. n_speech) is exactly what gsv_audio_convert gives for
 *   audio[begin .. end) alone -- the same fma chain, samples outside the span counting as zeros and
 *   never read as filter context; out[n_speech .. n_speech + pause_n) is zeros (+0.0f or int16 0);
 *   nothing beyond is written.  `out` must hold gsv_join_samples(n, out_rate, pause) =
 *   gsv_audio_samples(n, out_rate) + pause_n samples.
 *   Loudness: with a target, the measurement, the peak and the gain stay those of the whole
 *   untrimmed item (the gates already ignore silence); the gain multiplies the span's samples.
 *   `audio` (32 kHz float32) is still written, untrimmed and bit-unchanged.
 *   Span record: device int32[4] {begin, end, n_speech, n_out = n_speech + pause_n}, written on
 *   the device.  The same bits whatever the launch: alone, in a batch, on the vocoder's stream.
 * gsv_join rides beside an item as gsv_loudness does and carries its fields (target 0: no
 * loudness) plus trim: threshold in dBFS, 0 == off, valid -80 .. -20; pause: seconds, 0 == none,
 * valid 0 .. 5; span: device int32[4] or NULL.  Out of range is GSV_E_ARG before any launch.  An
 * item with a trim, a pause or a span needs `out`; a trim needs n <= 640 * 4096.  An item whose
 * gsv_join is all zero is the call without it: the same launches, the same bits. */
#define GSV_JOIN_FRAME 320
#define GSV_JOIN_GUARD 640
typedef struct { float target; float peak; float* stats; float trim; float pause; int32_t* span; } gsv_join;
/* Samples of `pause` seconds at out_rate, and the bound of `out` (see above); GSV_E_ARG for an
 * unsupported rate, a negative n_in or a pause outside 0 .. 5.  Pure: need no device. */
int gsv_join_pause_samples(int32_t out_rate, float pause);
int gsv_join_samples(int32_t n_in, int32_t out_rate, float pause);
/* The `_join` twins of the entries that take items: join is [n] (one per item; NULL: the plain
 * call).  The plain and the `_norm` entries forward here: one body, one set of checks.  A batch is
 * one frame pass and one span pass plus the stage launch per 256 items; after an fp16-range re-run
 * the re-run's audio is measured; under gsv_vits_decode_async_join all run on the vocoder's
 * stream.  join is copied: it need not outlive the call (the stats and span buffers must, until
 * the wait). */
int gsv_vits_decode_item_join(gsv_engine* eng, const gsv_vits_item* item, const gsv_join* join,
                              float noise_scale, void* stream);
int gsv_vits_decode_batch_join(gsv_engine* eng, int32_t n, const gsv_vits_item* items, const gsv_join* join,
                               float noise_scale, void* stream);
int gsv_vits_decode_batch_async_join(gsv_engine* eng, int32_t n, const gsv_vits_item* items,
                                     const gsv_join* join, float noise_scale, void* stream);
int gsv_vits_decode_async_join(gsv_engine* eng, const gsv_vits_item* item, const gsv_join* join,
                               float noise_scale, void* stream);
/* The stage alone: gsv_audio_convert (gsv_audio_normalize with a target) of the span of audio_32k
 * plus the pause; out holds gsv_join_samples(n_in, out_rate, join->pause).  join NULL: gsv_audio_convert. */
int gsv_audio_join(gsv_engine* eng, const float* audio_32k, int32_t n_in, const gsv_join* join,
                   int32_t out_rate, int32_t out_format, void* out, void* stream);
/* Debug: the frames' sums of squares (device double [ceil(n / 320)]) of audio (device f32 [n],
 * n <= 640 * 4096) alone, so the frame pass can be tested apart from the span logic. */
int gsv_debug_join_frames(gsv_engine* eng, const float* audio, int32_t n, double* sums, void* stream);

/* The T2S side of the same pipeline: encode + prefill the NEXT sentence ahead, on
 * the vocoder CUs while the current sentence decodes (the reference's per-sentence
 * encoder + first-stage decoder, Inference.py:63-72, moved off the critical path).
 * Needs option "vocoder_cus".  Call it for sentence i+1 before gsv_t2s_generate of
 * sentence i: it is queued and launched (into a spare KV slot, behind a queued
 * gsv_vits_decode_async call) right after that generate's decode kernel; the next
 * gsv_t2s_generate with batch 1 and a field-wise equal utt / sampler then decodes
 * from it (identical tokens).  A batch-1 generate of another utterance keeps a
 * queued prefetch; a batch generate or any other T2S call discards it.  The utt's
 * buffers must stay valid until the generate that uses it. */
int gsv_t2s_prefetch(gsv_engine* eng, const gsv_utt* utt, const gsv_sampler* sampler, void* stream);

/* gsv_t2s_generate for one utterance, split so the GPU never waits for the host
 * between the sentences of a stream: _start queues the utterance (taking its
 * prefetch when one matches) and returns at once; up to two may be in flight, so
 * the next decode is queued behind the running one.  _finish blocks for the oldest
 * started one and returns its trimmed tokens (host [out_stride]) as
 * gsv_t2s_generate would, ordering `stream` after it.  A launch that meets the
 * fp16-range or hand-off-timeout condition is re-run synchronously inside _finish.
 * Other T2S calls wait for the started ones first; their results stay queued.
 *
 * Decode lanes.  Under option "vocoder_cus" with at least 192 decode CUs (and option
 * "decode_lanes" at its default 2) the engine owns two decode lanes: CU-masked streams over
 * disjoint multiples of 32 of the decode CUs (192 -> 96 + 96, 224 -> 128 + 96), each with a
 * KV / sequence-state slot, hand-off ring and error word of its own.  A _start then takes
 * the lane whose previous generate was started least recently, so it may RUN BESIDE the
 * previous started generate instead of behind it: the sentences of a stream must be
 * independent (they are in the reference), and the utt's buffers of both must stay valid
 * until their _finish.  _finish still returns the results in the order of the starts.
 * The tokens are those of gsv_t2s_generate on either lane.  With fewer decode CUs, or
 * "decode_lanes" 1, there is one lane and a second start is queued behind the first.
 * Under two lanes the engine stream -- every synchronous or batched call under
 * "vocoder_cus" -- runs on lane 0's CUs only; a caller who mixes such calls into the
 * split and wants all decode CUs for them sets "decode_lanes" 1. */
int gsv_t2s_generate_start(gsv_engine* eng, const gsv_utt* utt, const gsv_sampler* sampler, void* stream);
int gsv_t2s_generate_finish(gsv_engine* eng, int64_t* out_tokens, int32_t out_stride, int32_t* out_len,
                            void* stream);

/* V2: the vocoder graph's reference branch alone (vits_fp32.onnx(v2)#79-271: refer
 * spectrogram -> MelStyleEncoder; ReferenceAudio.py:40-45 feeds it the 32 kHz audio on
 * every vocoder.run) -> ge (device [512]).  It depends on the reference only: pass it as
 * the ge of gsv_vits_decode or of a gsv_vits_item, with ref_audio NULL, for every sentence spoken
 * against that reference; the audio is identical to passing ref_audio. */
int gsv_ref_encode(gsv_engine* eng, const float* ref_audio, int32_t n_audio, float* ge, void* stream);

/* prompt_encoder_fp32.onnx (V2ProPlus): ref_audio (device [n_audio]),
 * sv_emb (device [20480]) -> ge (device [1024]), ge_adv (device [512]). */
int gsv_prompt_encode(gsv_engine* eng, const float* ref_audio, int32_t n_audio,
                      const float* sv_emb, float* ge, float* ge_adv, void* stream);

/* Timbre fusion: GPT-SoVITS's auxiliary reference clips (aux_ref_audio_paths; SynthesizerTrn.decode
 * with a list of references runs each clip through the reference encoder and averages the global
 * embeddings).  Each clip is encoded on its own, by gsv_ref_encode (V2, ge [512]) or by
 * gsv_prompt_encode with the clip's own sv_emb (V2ProPlus, ge [1024]), and the embeddings are
 * mixed here, once per reference set; the result is the ge of every vocoder entry.
 *   out[d] = sum_i weights[i] * ge[i][d], as one float32 chain per element in clip order:
 *     acc = weights[0] * ge[0][d];  acc = acc + weights[i] * ge[i][d]  (i = 1 .. n-1),
 *   every multiply and add rounded on its own (no fused multiply-add), so a restatement with
 *   float32 operations gives the same bits, and weights (1, 0, ..) give ge[0] value for value.
 * ge: HOST array of n device pointers (each [dim]), weights: HOST [n]; both are copied into the
 * launch's arguments and need not outlive the call.  The caller normalises the weights (the
 * Python layer: to sum 1 in float64, rounded once to float32; equal weights are GPT-SoVITS's
 * mean).  n in 1..GSV_MIX_MAX, dim in 1..4096, weights finite and >= 0 with at least one > 0,
 * else GSV_E_ARG (the message names the index) and nothing is launched.  out (device [dim]) may
 * be one of the inputs.  Stream-ordered, one launch, no workspace.  Either model version. */
#define GSV_MIX_MAX 16
int gsv_ge_mix(gsv_engine* eng, int32_t n, int32_t dim, const float* const* ge, const float* weights,
               float* out, void* stream);
/* V2ProPlus: ge_adv (device [512]) = ge_to512(ge (device [1024])), the last GEMV of
 * gsv_prompt_encode alone (the same call, so given gsv_prompt_encode's ge it returns
 * gsv_prompt_encode's ge_adv bit for bit).  The ge_adv of a fused voice is this projection of the
 * mixed ge, as in GPT-SoVITS, not a mix of the clips' ge_adv.  GSV_E_STATE on V2 or without
 * prompt-encoder weights. */
int gsv_ge_project(gsv_engine* eng, const float* ge, float* ge_adv, void* stream);

/* chinese-hubert-base.onnx (CN-HuBERT, ReferenceAudio.py:48-52; session loaded at
 * ModelManager.py:172-195): input_values = raw 16 kHz audio (device [n_samples])
 * -> ssl_content (device [768][T], the graph's [1, 768, T] output), T =
 * gsv_hubert_frames(n_samples) (the conv stack's output length).  Needs an
 * engine whose weights include the HuBERT tensors (transformers HubertModel
 * names, encoder.pos_conv_embed.conv.weight already weight-normed). */
int gsv_hubert_frames(int32_t n_samples);
int gsv_hubert(gsv_engine* eng, const float* audio_16k, int32_t n_samples, float* ssl_content, void* stream);

/* speaker_encoder.onnx (V2ProPlus speaker verification, ReferenceAudio.py:71-72:
 * speaker_verification_model.run(None, {'waveform': audio_16k}); session loaded at
 * ModelManager.py:155-170): waveform = the 16 kHz reference clip (device
 * [n_samples]) -> sv_emb (device [20480], the graph's [1, 20480] output), the
 * prompt encoder's sv_emb input.  Kaldi fbank (80 mel bins, 25/10 ms frames,
 * snip edges) -> ERes2NetV2 (GPT-SoVITS sv.py, baseWidth 24 / scale 4 / expansion 4)
 * forward3.  gsv_sv_frames(n) is the fbank frame count (0: too short, GSV_E_ARG).
 * Needs an engine whose weights include the SV tensors (weights.sv_spec names). */
int gsv_sv_frames(int32_t n_samples);
int gsv_sv(gsv_engine* eng, const float* audio_16k, int32_t n_samples, float* sv_emb, void* stream);

/* RoBERTa.onnx (chinese-roberta-wwm-ext-large BERT features for Chinese text,
 * GetPhonesAndBert.py:64-74; session ModelManager.py:132-150): input_ids (device
 * i64 [n_tokens], CLS .. SEP), attention_mask (host i64 [n_tokens], all ones, or
 * NULL), repeats = word2ph (host i64 [n_chars], n_chars <= n_tokens - 2) ->
 * text_bert (device [sum(repeats)][1024]) = hidden_states[-3] of the character
 * rows 1 .. n_chars, row i repeated repeats[i - 1] times.  Needs an engine whose
 * weights include the BertModel tensors (transformers names). */
int gsv_roberta(gsv_engine* eng, const int64_t* input_ids, const int64_t* attention_mask, int32_t n_tokens,
                const int64_t* repeats, int32_t n_chars, float* text_bert, void* stream);

/* The same for n_seq sentences in one pass (the reference runs RoBERTa once per
 * Chinese sentence; packed here: every GEMM over all sentences' token rows, attention
 * within each sentence): input_ids (device i64, the sentences' CLS .. SEP ids
 * concatenated), n_tokens (host [n_seq]), repeats (host i64, the sentences' word2ph
 * concatenated), n_chars (host [n_seq]) -> text_bert (device, the sentences'
 * [sum(word2ph_s)][1024] blocks concatenated in order).  Identical to n_seq gsv_roberta
 * calls. */
int gsv_roberta_batch(gsv_engine* eng, int32_t n_seq, const int64_t* input_ids, const int32_t* n_tokens,
                      const int64_t* repeats, const int32_t* n_chars, float* text_bert, void* stream);

/* Debug hooks (tests only): copy a named VITS workspace buffer after
 * gsv_vits_decode ("ge","stats","z","y","q","te","g0","g1","spec","a");
 * run one conv1d (zero padding) on device buffers; a non-NULL splitk_ws (device,
 * splitk_cap floats) enables the split-K path for under-filled grids. */
int gsv_debug_copy(gsv_engine* eng, const char* name, float* dst, int64_t n, void* stream);
int gsv_debug_conv1d(const float* x, int cin, int tin, const float* w, int cout, int k, int dil,
                     int pad, const float* bias, float* out, int tout, int in_act, float slope,
                     float* splitk_ws, int64_t splitk_cap, void* stream);
/* The speech-rate resample alone: x (device [c][t]) -> out (device [c][t_out]). */
int gsv_debug_interp_linear(const float* x, int c, int t, int t_out, float* out, void* stream);
/* The same conv on the f16-split MFMA path (vits_convh.hip, the MRF convs of
 * dec.resblocks.* in vits_fp32.onnx): wh = fp16 weights [cout][k][cin], scale =
 * per-output-channel f32 factor on the sums (weight norm g/||v||); *ovf (device
 * int) is OR-ed with 1 when an input exceeds the fp16 range.  GSV_E_ARG when the
 * shape is not covered (k in {3,7,11}, cin % 8 == 0, dil <= 5). */
int gsv_debug_conv1d_h(const float* x, int cin, int tin, const void* wh, const float* scale, int cout,
                       int k, int dil, int pad, const float* bias, float* out, int tout, int in_act,
                       float slope, int* ovf, void* stream);
/* The achievable HBM rate: `iters` grid-stride copies (16-B non-temporal
 * loads / stores, 4 per thread in flight) of `bytes`
 * (16-B aligned device buffers) on `stream`; *ms = the mean time of one copy (HIP events).
 * Read + write bytes = 2 x bytes per copy.  Measurement helper for bench.py. */
int gsv_debug_hbm_copy(const void* src, void* dst, int64_t bytes, int iters, void* stream, float* ms);
/* Phase timestamps (100 MHz) of the per-step-graph decode kernels (t2s_decode.hip:
 * the fp16-range re-run / timeout / B > 64 path, not the persistent kernels) of
 * layer 12, last step run: [kernel: QKV GEMV, attention, FFN][block 0..255][slot
 * 0..7]; needs GENIE_KTRACE=1 in the environment at gsv_finalize_weights. */
int gsv_debug_ktrace(gsv_engine* eng, uint64_t* host, int n);
/* Run the decode sampler kernel once on logits (device [B][1025]) with the
 * token-presence bitmaps seen (device u32 [B][33]) at loop step `step`
 * (Philox counter); tokens (device i64 [B]) and stop flags (device u8 [B]). */
int gsv_debug_sample(const float* logits, const uint32_t* seen, int B, const gsv_sampler* s,
                     int step, int64_t* tokens, uint8_t* stop, void* stream);
/* The same launch with a per-row sampler table (gsv_t2s_generate_each): samplers (host [B]),
 * streams (host [B], or NULL: streams[b] = b). */
int gsv_debug_sample_each(const float* logits, const uint32_t* seen, int B, const gsv_sampler* samplers,
                          const int32_t* streams, int step, int64_t* tokens, uint8_t* stop, void* stream);

/* One launch of the engine's GEMM entry (gemm_nt, csrc/t2s.hip) on device buffers, engine-free:
 * C(m,n) = epi(sum_k A[m lda + k] W[n ldw + k] + bias[n]).  Every pointer is a device pointer, 0
 * where the launch has none.
 *   w_kind: 0 f32 weights in w; 1 fp16 weights in w; 2 split fp32 weights, fp16 hi plane in w and
 *     lo plane in wl (lo = fp16((w - hi) 2^11)).
 *   mode: 0 store, 1 relu, 2 res + v, 3 q columns + K/V-cache scatter (kv_*), 4 VQ distance
 *     (rowsq, colsq), 5 mish, 6 split-K slabs (ksplit, slab_stride; no bias), 7 gelu, 8 relu as fp16
 *     hi / lo planes (ch, cl; no c).
 *   a_nslab > 0: A = relu?(a_bias + the sum of a_nslab slabs a_slab_stride apart).  ah / al: A's fp16
 *     hi / lo planes (large-M form only).  cus / small_ns: the stream's CUs and a forced small-M ring
 *     depth (0, 2, 3, 4), host only.
 *   dry != 0: check the arguments and report the form, launch nothing (no HIP call).
 * *form = the kernel that ran (or would): 0 generic f32, 1 generic f16, 2 x2, 3 / 4 / 5 small-M with
 * 2 / 3 / 4 stages, 6 large-M, 7 large-M with pre-split A, 8 split weights.
 * GSV_E_ARG, before any HIP call, for an argument set the kernels' loads and stores do not cover:
 * null or misaligned pointers, K % 32, leading dimensions, a mode on a path that has no such
 * epilogue (gsv_last_error names it). */
typedef struct gsv_gemm_desc {
    int32_t M, N, K, w_kind, mode, dry;
    const float* a; int64_t lda;
    const void* w; const void* wl; int64_t ldw;
    const float* bias;
    float* c; int64_t ldc;
    const float* res; int64_t ldr;
    const float* rowsq; const float* colsq;
    float* kv_k; float* kv_v; int32_t kv_tmax, kv_pos0;
    const int32_t* kv_row_pos; int64_t kv_seq_stride; const int32_t* kv_row_seq; const uint8_t* kv_row_skip;
    int32_t ksplit, a_nslab; int64_t slab_stride, a_slab_stride;
    const float* a_bias; int32_t a_relu, cus;
    const void* ah; const void* al; void* ch; void* cl;
    int32_t small_ns, reserved;
} gsv_gemm_desc;
int gsv_debug_gemm(const gsv_gemm_desc* d, void* stream, int32_t* form);
/* One launch of a row kernel of csrc/t2s.hip / csrc/hubert.hip on device buffers.
 *   op 0 layernorm_rows (D = 512, eps 1e-5): in -> out [rows][512] with g, b.
 *   op 1 layernorm_rows_slabs: LayerNorm of res + (bias + sum of nslab slabs of `in`, slab_stride
 *     apart); out_hi / out_lo (optional, both or neither) take the fp16 split of out.
 *   op 2 layernorm_rows_d, op 3 layernorm_rows_d_slabs: the same over D <= 1024 with eps.
 *   op 4 sumsq_rows: out[r] = sum_c in[r ld + c]^2, c < D.
 *   op 5 argmin_dist_rows: out (int64 [rows]) = the first index of the least of in[r D + c], c < D.
 * rows == 0 returns 0 without a launch; GSV_E_ARG before any HIP call for null pointers or sizes
 * the kernel does not cover. */
typedef struct gsv_rows_desc {
    int32_t op, rows, D, nslab;
    const float* in; void* out; int64_t ld, slab_stride;
    const float* g; const float* b; const float* bias; const float* res;
    void* out_hi; void* out_lo;
    float eps; int32_t reserved;
} gsv_rows_desc;
int gsv_debug_rows(const gsv_rows_desc* d, void* stream);

/* One launch of the vocoder's conv entry (conv1d / conv1d_deferred, csrc/vits.hip) on device
 * buffers, engine-free; the fields are those of ConvArgs (csrc/vits.h), which states the operation.
 * Every pointer is a device pointer, 0 where the launch has none.
 *   wh != 0: the f16-split path (k_conv_h / k_conv_ws), refused where it does not cover the shape;
 *     wh == 0: the f32 kernel on w.
 *   n_x, n_w, n_out, n_res, n_acc, n_out2, n_seg: the element counts of x, w (or wh), out, res, acc,
 *     out2 (= res2) and seg as the caller allocated them; part_cap that of part.
 *   dry != 0: check the arguments and report the form, launch nothing (no HIP call).
 *   deferred != 0: conv1d_deferred; form[3] = the slab count it left in part (0: out is complete).
 * form[0] = the path (1 f32 direct, 2 f32 split-K, 3 k_conv_h, 4 k_conv_ws); f32: form[1] = nsplit,
 * form[2] = 1 with float4 weight loads; f16: form[1] = the channel chunk (32 / 8), form[2] = the tile
 * candidate 0..3.
 * GSV_E_ARG, before any HIP call: K outside the instantiated set, dil outside 1..5, a null pointer
 * the mode dereferences, div == 0 for mode 8, seg with deferred, extents (n_t, o_tstride, o_toff,
 * phases, o_len, strides) past the stated element counts, and on the f16 path a misaligned wh,
 * Cin % 8 != 0 or x_ts != 1 (gsv_last_error names it). */
typedef struct gsv_conv_desc {
    int32_t Cin, Tin, Cout, K, dil, pad;
    int32_t n_t, o_tstride, o_toff, o_len;
    int32_t in_act, mode, split, phases;
    int32_t tile_force, ws, dry, deferred;
    float in_slope, div;
    const float* x; int64_t x_cs, x_ts;
    const float* w; const float* bias;
    float* out; int64_t o_cs, o_ts;
    const float* res; int64_t r_cs, r_ts;
    const float* vec; float* acc; float* out2; const float* res2;
    int64_t w_phase_stride;
    float* part; int64_t part_cap;
    const void* wh; const float* wscale; int32_t* ovf; int64_t wh_phase_stride; const float* in_scale;
    const int32_t* seg; int64_t vec_sstride;
    int64_t n_x, n_w, n_out, n_res, n_acc, n_out2, n_seg;
} gsv_conv_desc;
int gsv_debug_conv(const gsv_conv_desc* d, void* stream, int32_t form[4]);
/* One fused ResBlock step (mrf_pair, csrc/vits_mrf.hip): the fields of MrfPairArgs and of its
 * epilogue ConvArgs (res = r); n_r, n_out, n_acc the element counts of r, out and acc.  GSV_E_ARG
 * with mrf_pair's reason where it does not cover the arguments, for a null buffer the mode uses,
 * out aliasing r, misaligned weights and buffers smaller than C x T. */
typedef struct gsv_mrf_desc {
    int32_t T, C, K, dil, mode, Cout, n_t, o_len, o_tstride, o_toff;
    float div; int32_t reserved;
    const float* r;
    const void* w1; const float* s1; const float* b1;
    const void* w2; const float* s2; const float* bias2;
    int32_t* ovf;
    float* out; float* acc; const int32_t* seg;
    int64_t o_cs, o_ts, r_cs, r_ts;
    int64_t n_r, n_out, n_acc, n_seg;
} gsv_mrf_desc;
int gsv_debug_mrf_pair(const gsv_mrf_desc* d, void* stream);
/* One launch of the vocoder's attention (mha, csrc/vits.hip): the fields of MhaArgs; row_seg_host
 * = the host copy of row_seg ([nq][2], required with it); n_q, n_k, n_v, n_out the element counts.
 * GSV_E_ARG: dk > 128, a row's key count outside 1..2048, window > 8, rel-pos terms with
 * nq != nk and no row_seg (or a row outside its own key range), key ranges or strides that leave
 * a buffer. */
typedef struct gsv_mha_desc {
    int32_t nq, nk, heads, dk, postdiv, window;
    float scale; int32_t reserved;
    const float* q; int64_t q_ts, q_cs;
    const float* k; int64_t k_ts, k_cs;
    const float* v; int64_t v_ts, v_cs;
    float* out; int64_t o_ts, o_cs;
    const float* ek; const float* ev;
    const int32_t* row_seg; const int32_t* row_seg_host;
    int64_t n_q, n_k, n_v, n_out;
} gsv_mha_desc;
int gsv_debug_mha(const gsv_mha_desc* d, void* stream);
/* One launch of a row kernel of csrc/vits.hip on [C][T] device buffers.
 *   op 0 ln_channels: out = LN_C(x + y) (y, seg optional) with g, b.
 *   op 1 ln_channels_slabs: y = bias + the nsplit slabs [nsplit][C][T] in `y` (bias optional).
 *   op 2 wn_gate: out [C][T] = tanh(x[c]) sigmoid(x[C + c]), x [2C][T].
 *   op 3 wn_gate_slabs: the same of (bias + the nsplit slabs [nsplit][2C][T] in x) + vec (per seg).
 *   op 4 mean3: out = ((x + y) + z) / div over n elements.
 *   op 5 seg_fill: out (int32 [n]) from off, len (device int32 [nseg]) and the factor f.
 * T == 0 (n == 0) returns 0 without a launch.  GSV_E_ARG for what the host entries abort on or
 * cannot cover: C outside 1..256, seg or slabs with C % 16 != 0, nsplit < 2 (op 1) / < 1 (op 3),
 * null pointers, nseg < 1, f < 1. */
typedef struct gsv_vits_rows_desc {
    int32_t op, C, T, nsplit, nseg, f;
    int64_t n, vec_sstride;
    float div; int32_t reserved;
    const float* x; const float* y; const float* z; void* out;
    const float* g; const float* b; const float* bias; const float* vec;
    const int32_t* seg; const int32_t* off; const int32_t* len;
} gsv_vits_rows_desc;
int gsv_debug_vits_rows(const gsv_vits_rows_desc* d, void* stream);

/* One launch of a T2S attention kernel (csrc/t2s.hip) on device buffers, engine-free.  16 heads of
 * 32 dims; q [rows][ldq], K / V caches [16][tmax][32] per sequence, seq_stride elements apart;
 * row r attends over keys [0, row_len[r] + len_add) of sequence row_seq[r] (0 without row_seq).
 *   form 0 auto: attn_rows; *form = the kernel its rule (attn_form) picked, 1 or 2.
 *   form 1 rows: k_attn_rows (attn_rows_plus with len_add, 0 allowed).  form 2 flash: k_attn_flash,
 *     blocks of 16 rows or the tiles.  form 3 rowlane / 4 mf32: the packed-prefill kernels over
 *     `tiles` ([ntiles][3] {sequence, first row, rows}).  form 5 dec_slabs: attn_decode_slabs;
 *     rows = B, row_len = kvlen, row_skip = done, q = b_in + the sum of nslab slabs [B][1536]
 *     slab_stride apart, the new K / V row appended at kvlen[b]; out [B][512].
 *   row_len_host, row_seq_host, tiles_host: host copies of the device arrays (required with them):
 *     the hook checks those.  len_add is form 1's alone and must be 0 elsewhere.
 *   dry != 0: check and report the form, launch nothing (no HIP call).
 * GSV_E_ARG before any HIP call: rows or tmax <= 0, a null buffer, a length outside [1, tmax] (or
 * above 4096 for forms 1 and 5), q / k / v not 16-B aligned, ldq % 4, ldo % 4 or an unaligned out
 * (forms 3, 4), seq_stride % 4 or below one cache with several sequences, forms 3 / 4 without
 * tiles, a tile of more rows than a block holds (16 flash, 128 rowlane, 128 mf32), past `rows` or of
 * a negative sequence, flash or auto-with-tiles misuse (gsv_last_error names it), and for form 5
 * nslab < 1, null b_in / kvlen / done, kvlen[b] + 1 > tmax, overlapping slabs. */
typedef struct gsv_attn_desc {
    int32_t form, rows, tmax, len_add, ntiles, nslab, dry, reserved;
    float scale; int32_t reserved2;
    const float* q; int64_t ldq;
    float* k; float* v; int64_t seq_stride;
    const int32_t* row_len; const int32_t* row_len_host;
    const int32_t* row_seq; const int32_t* row_seq_host;
    const uint8_t* row_skip;
    float* out; int64_t ldo;
    const int32_t* tiles; const int32_t* tiles_host;
    const float* slabs; int64_t slab_stride; const float* b_in;
} gsv_attn_desc;
int gsv_debug_attn(const gsv_attn_desc* d, void* stream, int32_t* form);
/* One attn_outproj launch (csrc/t2s_decode.hip): sequence b attends over [0, kvlen[b] + 1) and the
 * head's out-projection partial goes to part [16][B][512], or as fixed point (2^-32) into
 * acc_out [b * acc_bstride + n].  GSV_E_ARG: B <= 0, null tensors, kvlen_host[b] + 1 outside
 * [1, tmax], q / k / v / WoT not 16-B aligned, both or neither of part / acc_out, acc_bstride < 512
 * with B > 1, seq_stride below one cache with B > 1. */
typedef struct gsv_attn_out_desc {
    int32_t B, tmax; float scale; int32_t reserved;
    const float* q; const float* k; const float* v; int64_t seq_stride;
    const int32_t* kvlen; const int32_t* kvlen_host; const uint8_t* done;
    const void* WoT; float* part; int64_t* acc_out; int64_t acc_bstride;
} gsv_attn_out_desc;
int gsv_debug_attn_out(const gsv_attn_out_desc* d, void* stream);
/* One gemv_f16 launch (csrc/t2s.hip): the fields of GemvArgs; kv_row_pos_host the host copy of
 * kv_row_pos.  mode: 0 store, 1 relu, 2 resid, 3 qkv.  GSV_E_ARG: B outside [1, 8], K not 512 or
 * 2048, N <= 0, a LayerNorm prologue (ln_g) with K != 512 or without ln_b, part / acc_in without
 * ln_g (or both, or without part_bias / part_res), n_part no positive multiple of 16, a plain
 * prologue with lds % 4 or an unaligned or null src, W not 16-B aligned, null C, resid without res,
 * qkv with N != 1536, without caches or with a position outside [0, kv_tmax), another mode. */
typedef struct gsv_gemv_desc {
    int32_t B, N, K, mode, n_part, kv_tmax, kv_pos0, reserved;
    const float* src; int64_t lds;
    const float* part; int64_t part_stride; const float* part_bias; const float* part_res;
    const int64_t* acc_in; int64_t acc_bstride;
    const float* ln_g; const float* ln_b; float* ln_out;
    const void* W; const float* bias;
    float* C; int64_t ldc;
    const float* res; int64_t ldr;
    float* kv_k; float* kv_v; int64_t kv_seq_stride;
    const int32_t* kv_row_pos; const int32_t* kv_row_pos_host; const uint8_t* kv_row_skip;
} gsv_gemv_desc;
int gsv_debug_gemv(const gsv_gemv_desc* d, void* stream);
/* One ffn_fused launch (csrc/t2s_decode.hip): the fields of FfnArgs; the attention hand-off comes
 * as floats (attn_part [16][B][512]) or fixed point (acc_attn), the result leaves as floats
 * (part [nslices][B][512]) or fixed point (acc_out).  GSV_E_ARG: nslices not 32 or 64, B outside
 * [1, 8], null tensors, both or neither of each hand-off pair, W1 / W2T not 16-B aligned,
 * acc_bstride < 512 with B > 1 and a fixed-point hand-off. */
typedef struct gsv_ffn_desc {
    int32_t B, nslices;
    const float* h; const float* bo; const float* attn_part; const int64_t* acc_attn;
    const float* ln_g; const float* ln_b; float* h1;
    const void* W1; const float* b1; const void* W2T;
    float* part; int64_t* acc_out; int64_t acc_bstride;
} gsv_ffn_desc;
int gsv_debug_ffn(const gsv_ffn_desc* d, void* stream);
/* One launch of an exact f32 embedding kernel of csrc/t2s.hip.
 *   op 0 decode_embed: out[b] = emb[tok[b][ny[b] - 1]] + alpha pe[ny[b]] for n = B sequences
 *     (tok [B][ldy] int64, done optional); tok_host / ny_host the host copies.
 *   op 1 audio_embed_prompts: out[p] = emb[tok[p]] + alpha pe[p + 1], p < n.
 *   op 2 ssl_im2col: out[t][2 ci + j] = ssl[ci][2 t + j], ci < 768, t < n / 2 (n = n_ssl).
 * emb is fp16 [n_tok][512], pe [n_pe][512].  GSV_E_ARG: n <= 0, null tensors, a token outside
 * [0, n_tok), ny[b] outside [1, ldy] or a pe row at or past n_pe. */
typedef struct gsv_embed_desc {
    int32_t op, n, n_tok, n_pe;
    const int64_t* tok; const int64_t* tok_host; int64_t ldy;
    const int32_t* ny; const int32_t* ny_host;
    const void* emb; const float* alpha; const float* pe;
    float* out; const uint8_t* done; const float* ssl;
} gsv_embed_desc;
int gsv_debug_embed(const gsv_embed_desc* d, void* stream);

/* Probe: replay one kernel configuration `iters` times (hipGraph) between HIP
 * events on the engine stream; *us = average microseconds per launch.
 * which: 0/1 empty kernel (1/256 blocks), 2 QKV GEMV (+LN prologue), 3 QKV GEMV,
 * 4 FFN1 GEMV (+LN), 5 FFN2 GEMV, 6 out-proj GEMV, 7 decode attention,
 * 8 one full decode step (graph) for batch B.  Requires gsv_reserve(B, ...). */
int gsv_probe(gsv_engine* eng, int which, int B, int iters, float* us, void* stream);

/* Per-phase device time of the last gsv_t2s_generate / gsv_vits_decode (ms):
 * [0]=encode [1]=prefill [2]=decode [3]=vits.  Filled when timing is enabled. */
int gsv_set_timing(gsv_engine* eng, int enabled);
int gsv_get_timing(gsv_engine* eng, float* ms4);
/* Live duration of the dominant kernel, the persistent decode launch (k_decode_persist1 /
 * k_decode_persist1m: the whole decode loop of a generate): while timing is enabled each
 * launch carries start/stop events stamped from its dispatch packet
 * (hipExtLaunchKernelGGL).  On the per-step graph path the sample is one eagerly run step's
 * FFN launch instead.  Average microseconds and number of samples; a negative count is
 * -(hipError_t) of a failed hipEventElapsedTime. */
int gsv_get_kernel_timing(gsv_engine* eng, float* avg_us, int32_t* samples);

/* Stop (the reference's GENIE.stop_event, checked before every loop step:
 * Inference.py:96-97 returns None for the sentence).  on = 1 sets the engine's stop
 * word, 0 clears it (TTSPlayer.py:86 clears the event when a new job starts).  While it
 * is set, T2S generates (gsv_t2s_generate, _start/_finish) return GSV_E_STOPPED: a
 * running decode leaves within two loop steps -- the persistent kernels read the word
 * once per step at token resolution, the per-step graphs' sampler every step -- and a
 * new one returns at once.  The engine stays usable.  The only entry point that may be
 * called from another thread while a call on the engine runs: it writes one word. */
int gsv_request_stop(gsv_engine* eng, int32_t on);

/* Engine options (no reference counterpart; the reference's session options are
 * ORT's).  "persist": 1 (default) runs gsv_t2s_generate's decode loop as ONE
 * persistent launch (B <= 64), 0 as replayed per-step hipGraphs; setting it also ends
 * a timeout back-off.  "persist1m" (1): B = 2..64 on the multi-sequence kernel (0: the
 * graphs); "persistm" (1) / "persistm_min_b" (32): from that batch size on, the batched
 * kernel with the batch on the MFMA M dimension (t2s_persistm.hip; groups of <= 4
 * sequences per 16 CUs).  "persist_backoff" / "persist_backoff_ms": the first back-off hold
 * after two timed-out launches in a row (64 generates / 5 s, doubling per failed re-probe).
 * "vocoder_cus" (CU split for the sentence pipeline), "decode_cus" / "decode_cu_offset",
 * "decode_lanes" (2, default: two decode lanes under "vocoder_cus" wherever >= 192 decode CUs
 * hold them, see gsv_t2s_generate_start; 1: one lane, a second started generate queued behind
 * the first; set with no generate started), "prefetch_first" (0, default; 1: with two lanes a
 * queued prefetch is launched before the queued vocoder call -- measured equal),
 * "vits_lanes", "seg_vocoder" (1, default: a vocoder batch runs its generator as ONE pass
 * over all utterances laid out back to back), "seg_front" (1, default: its text/flow part
 * too, see gsv_vits_decode_batch), "convh" (MRF convs on the split-fp16 MFMA),
 * "convt_f16" (1, default: the upsample ConvTransposes on it too), "mrf_fused" (1, default:
 * each conv pair of an MRF resblock step of the C <= 32 stages as one kernel, its
 * intermediate in LDS), "sv_f16", "packed", "attn_mf32" (1, default: the prefill's
 * attention on the f32 MFMA with k_attn_flash's exact fma chains; 0: k_attn_flash itself,
 * bit-identical results), "vits_fork" (1, default: a single VITS call on the engine's unmasked
 * stream runs the front's text branch beside its SSL branch and a generator stage's three resblocks
 * on three streams; 0: in order on one stream; bit-identical),
 * "pf_delay" (0: a B = 1 decode workgroup waits N x s_sleep(32)
 * between its publish and its next-layer refill),
 * "convh_ws" (the 7- / 11-tap MRF convs with 64 / 128 input channels weight-stationary, k_conv_ws:
 * 2 -- the default -- in a synchronous gsv_vits_decode_batch, whose vocoder has the GPU to
 * itself; 1 in every batched generator pass; 0 off; bit-identical),
 * "gemm_small_ns" (ring depth of the small-M fp16-weight GEMM form: 0, the default, follows the
 * launch's grid and the CUs of its stream -- a prefill on the vocoder CUs takes a shallower
 * ring, so two or three blocks share a CU; 2 / 3 / 4 forced; bit-identical),
 * "vits_slab_fuse" (1, default: the vocoder front's LayerNorms after an attention out-projection
 * or FFN2 and its WaveNet gates sum the split-K slabs of the conv before them; 0: that conv
 * launches its own reduce; bit-identical),
 * A/B options measured and left off: "vocoder_first" (a batched decode waits for the running
 * vocoder batch), "lanes_all_cus" (under vocoder_cus, the batch lanes on every CU),
 * "knob0".."knob3" (decode tuning variants),
 * test hooks ("persist_spin_ticks", "persist1_f16_limit", "sv_f16_limit", "convh_tile":
 * 1..4 forces that k_conv_h tile candidate, 0 the cost model).  "ptrace": 1 allocates per-workgroup phase stamps of the persistent
 * launch (step 8, layer 12), read back with gsv_debug_ptrace ([256 workgroups][16
 * slots]: 8 stamps of the 100 MHz clock, then the same 8 of the shader clock).
 * GSV_E_ARG for an unknown name. */
int gsv_set_option(gsv_engine* eng, const char* name, int value);
/* Engine counters: "persist_timeouts" (persistent decode launches whose hand-offs
 * timed out -- e.g. other work on the device -- and re-ran as per-step graphs),
 * "persist_disabled" (back-off holds begun), "persist_hold" (generates left in the
 * current hold), "persist_launches", "decode_lanes" (1 or 2: the decode lanes as currently
 * configured), "lane_launches_0" / "lane_launches_1" (persistent launches issued on each
 * lane; the synchronous paths count on lane 0), "persist1_f16_reruns" (fp16-range fallbacks),
 * "vits_f32_reruns", "vits_packed_fronts" (vocoder batches whose text/flow part ran
 * packed), "vits_slab_consumers" (LayerNorm / gate launches of the vocoder front that summed
 * the split-K slabs of the conv before them, option "vits_slab_fuse"), "sv_f32_reruns", "w16_split_tensors" (fp32 weights kept as hi + lo
 * planes), "stops" (generates abandoned by gsv_request_stop), "graph_fallbacks"
 * (per-step decode loops run eagerly because their hipGraph capture failed -- e.g.
 * invalidated by another thread's device-wide synchronisation), "retired_bytes" (device
 * buffers replaced by a capacity growth and not yet freed), "reclaimed_bytes" / "reclaims"
 * (freed by the growth paths once the engine's streams drained; capacities grow in
 * quantised steps: batch to a power of two, tokens to a multiple of 256, workspaces by
 * 1.25x, so a load ramp re-allocates a few times and keeps no dead copies). */
int gsv_get_counter(gsv_engine* eng, const char* name, int64_t* value);
int gsv_debug_ptrace(gsv_engine* eng, uint64_t* host, int n);

#ifdef __cplusplus
}
#endif
#endif /* GENIE_ENGINE_H */
