/* gsv.h -- C ABI of libgsv_hip.so, the MI355X (gfx950) GPT-SoVITS synthesis hot path.
 *
 * Drop-in boundary.  Each group of entry points replaces one seam
 * of the reference (paths under /root/reference/GPT_SoVITS):
 *
 *   gsv_t2s_*    <- Text2SemanticDecoder.infer_panel_batch_infer / infer_panel_naive
 *                   AR/models/t2s_model.py:583-779, 814-918 (called from
 *                   TTS_infer_pack/TTS.py:1215-1227 and inference_webui.py:878);
 *                   sampling AR/models/utils.py:140-199
 *   gsv_vits_*   <- SynthesizerTrn.decode / extract_latent, module/models.py:961-1010
 *                   (called from TTS_infer_pack/TTS.py:1271, 818; inference_webui.py:920)
 *   gsv_bwe_*    <- tools/audio_sr.py::AP_BWE.__call__ (AP-BWE 24k -> 48k super-sampling, called from
 *                   TTS_infer_pack/TTS.py:1407-1417 when super_sampling is requested for v3)
 *   gsv_aa_act_forward <- anti_alias_activation_cuda.forward, the reference's only native
 *                   FFI: BigVGAN/alias_free_activation/cuda/anti_alias_activation.cpp:19-22,
 *                   anti_alias_activation_cuda.cu:212-246
 *   gsv_op_*     <- single kernels exposed for parity tests
 *
 * Conventions: plain C, no torch types.  Pointers marked [dev] are device (HBM) pointers owned
 * by the caller; [host] are host pointers.  `stream` is a hipStream_t passed as void*.
 * Every function returns GSV_OK (0) or a negative error code; gsv_last_error() returns a
 * thread-local message.  Handles are re-entrant per handle: one handle, one stream at a time.
 * There is no CPU fallback: every entry point fails with GSV_ERR_HIP if no gfx950 device exists.
 */
#ifndef GSV_H_
#define GSV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSV_OK 0
#define GSV_ERR_ARG (-1)
#define GSV_ERR_HIP (-2)
#define GSV_ERR_STATE (-3)

#define GSV_F32 0 /* fp32 storage, exact-f32 MFMA: parity mode                      */
#define GSV_F16 1 /* fp16 storage, fp32 accumulation: production mode (is_half=True) */

typedef void* gsv_stream_t;

int gsv_init(int device);
const char* gsv_last_error(void);
int gsv_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * AR semantic-token decoder (H1-H5)
 * ------------------------------------------------------------------------------------- */
typedef struct gsv_t2s gsv_t2s_t;

typedef struct {
  int n_layer;        /* 24 */
  int dim;            /* 512 */
  int n_head;         /* 16 */
  int ffn_dim;        /* 4*dim (t2s_model.py:304) */
  int vocab;          /* 1025, EOS = vocab-1 */
  int phoneme_vocab;  /* 732 (v2) / 512 (v1) */
  int bert_dim;       /* 1024 */
} gsv_t2s_config;

typedef struct {
  int top_k;                /* <=0: disabled */
  float top_p;              /* >=1: disabled */
  float temperature;
  float repetition_penalty;
  int early_stop_num;       /* -1: none; else stop once generated > early_stop_num (t2s_model.py:747) */
  int eos_mask_steps;       /* EOS column dropped while step < this: 1 for the batched loop
                               (t2s_model.py:708-710), 11 for infer_panel_naive (:888-889) */
  int max_steps;            /* reference hard cap 1500 (t2s_model.py:701) */
  uint64_t seed;            /* counter-RNG key for the Exp(1) race when no noise is injected */
} gsv_sampling_params;

int gsv_t2s_create(const gsv_t2s_config* cfg, int dtype, int max_batch, int max_seq, gsv_t2s_t** out);
void gsv_t2s_destroy(gsv_t2s_t* h);
/* name = reference state-dict key without the "model." prefix;
 * data [host] fp32, numel elements. */
int gsv_t2s_load_tensor(gsv_t2s_t* h, const char* name, const float* data, int64_t numel);
int gsv_t2s_finalize(gsv_t2s_t* h);

/* Prefill (H2+H3): phones [dev] int32 packed, phone_lens [host] int32[B], bert [dev] fp32
 * [sum(X_b)][bert_dim] row-major (token-major; NULL = all zeros, the non-zh path), prompts [dev]
 * int32 [B][P]; P == 0 (prompts may be NULL) is the reference's prompt-free mode (t2s_model.py:849-856: the audio sequence
 * starts empty at position 0).  Leaves the KV cache and per-row state ready for gsv_t2s_decode. */
int gsv_t2s_prefill(gsv_t2s_t* h, const int32_t* phones, const int32_t* phone_lens, int B,
                    const float* bert, const int32_t* prompts, int P, gsv_stream_t stream);
/* Prefill of a batch whose rows carry prompts of different lengths (one reference voice per row): prompts_packed [dev]
 * int32, row b's P_b = prompt_lens[b] [host] tokens back to back in row order; every P_b >= 1 (prompt-free rows keep
 * gsv_t2s_prefill with P = 0).  Row b needs phone_lens[b] + P_b + 2 <= max_seq; its generated tokens sit at audio
 * positions P_b, P_b + 1, ... and its repetition history is its own prompt plus what it generated.  With every P_b equal
 * this computes exactly what gsv_t2s_prefill computes.
 * After gsv_t2s_set_row_limits (pending for the decode that follows; B must match) a row may be prompt-free, P_b == 0: it has
 * no entry in prompts_packed, its audio sequence starts empty at position 0 and its EOS horizon is its limits' (the
 * reference's prompt-free loop uses 11); prompts_packed may be NULL when every row is prompt-free.  The same holds for
 * gsv_t2s_session_admit.  Without pending limits P_b == 0 is refused as before. */
int gsv_t2s_prefill_ragged(gsv_t2s_t* h, const int32_t* phones, const int32_t* phone_lens, int B, const float* bert,
                           const int32_t* prompts_packed, const int32_t* prompt_lens, gsv_stream_t stream);
/* Counter-RNG keys for the NEXT gsv_t2s_decode call only (like gsv_t2s_set_debug): row b draws with the key
 * (seeds[b], rows[b]) [host] instead of (sp->seed, b), so a row draws the same tokens wherever it sits in a batch.
 * B must equal the batch of that call.  Without it the keys are (sp->seed, b).  The key holds 24 bits of the row (DESIGN.md
 * section 4d, "The counter RNG as a contract"): a row outside [0, 2^24) is refused with GSV_ERR_ARG and nothing is kept, here and
 * in gsv_t2s_session_admit. */
int gsv_t2s_set_row_rng(gsv_t2s_t* h, const uint64_t* seeds, const int32_t* rows, int B);

/* Sampling parameters of one batch row: the four per-request fields of gsv_sampling_params. */
typedef struct {
  int top_k;                /* 0 = off */
  float top_p;              /* 0 < top_p <= 1; 1 = off */
  float temperature;        /* finite, >= 0 (clamped at 1e-5 like the scalar) */
  float repetition_penalty; /* finite, > 0; exactly 1 = off for this row */
} gsv_row_sampling_t;

/* Per-row sampling parameters for the NEXT gsv_t2s_decode call only (like gsv_t2s_set_row_rng): row b samples with
 * rows[b] [host] instead of the call's top_k / top_p / temperature / repetition_penalty, which are then ignored; everything
 * else still comes from the call's gsv_sampling_params.  B must equal the batch of that call.  A value outside the ranges
 * above is refused here with GSV_ERR_ARG and nothing is kept.  Without this call every row uses the scalars. */
int gsv_t2s_set_row_sampling(gsv_t2s_t* h, const gsv_row_sampling_t* rows, int B);

/* Step limits of one batch row: the three limit fields of gsv_sampling_params. */
typedef struct {
  int eos_mask_steps;       /* >= 0: EOS column dropped while the row's step < this */
  int early_stop_num;       /* -1: none; else >= 0, the row stops once it generated > early_stop_num */
  int max_steps;            /* >= 1 and <= the max_steps of the call / session: the row ends at step max_steps - 1 at the latest */
  int reserved;             /* 0 */
} gsv_row_limits_t;

/* Per-row limits for the NEXT gsv_t2s_decode call or the NEXT gsv_t2s_session_admit only (like gsv_t2s_set_row_rng and
 * gsv_t2s_set_row_sampling): row b masks EOS, stops early and ends by rows[b] [host] instead of the call's (session's)
 * eos_mask_steps / early_stop_num / max_steps.  The call's max_steps stays the row pitch of out_tokens, of the
 * log-probabilities and of the debug hooks, and a row that reaches its own budget ends like a row that reaches the scalar one:
 * out_len[b] and its last log-probability are written.  The arena, position-table and history checks are made per row with
 * budget_b = min(max_steps_b, early_stop_num_b + 1): phone_lens[b] + P_b + 2 + budget_b <= max_seq.
 * Call it BEFORE the prefill of that decode: a gsv_t2s_prefill_ragged (or an admission) that follows it accepts prompt-free
 * rows (see there).  GSV_ERR_ARG with nothing kept: eos_mask_steps < 0, early_stop_num < -1, max_steps < 1, reserved != 0,
 * B outside 1 .. max_batch; the consuming call refuses, before any launch and dropping the limits, a B different from its
 * rows and a max_steps above its own.  A session keeps a slot's limits with the slot's row state until the row is finished or
 * released; a row admitted without limits runs by the session's scalars.  Without this call every row runs by the scalars of the
 * call: the engine fills the rows' limits with them, and the kernels read only the rows'. */
int gsv_t2s_set_row_limits(gsv_t2s_t* h, const gsv_row_limits_t* rows, int B);

/* Decode loop (H4+H5).  noise [dev] fp32 Exp(1) draws [max_steps][noise_rows][vocab] or NULL
 * (noise_rows is 1 = shared by all rows, or B).  out_tokens [dev] int32 [B][max_steps]: generated
 * tokens (the finishing EOS / overflow token is not counted); out_len [dev] int32 [B] = the
 * reference's idx_list.  steps_run [host] receives the number of steps executed. */
int gsv_t2s_decode(gsv_t2s_t* h, const gsv_sampling_params* sp, const float* noise, int noise_rows,
                   int32_t* out_tokens, int32_t* out_len, int* steps_run, gsv_stream_t stream);

/* Decode sessions: continuous batching of the AR decode.  A session owns `slots` rows of the handle's K/V arena; rows are admitted
 * into free slots, all live rows advance together a chunk of steps at a time, and a slot whose row has finished can be admitted
 * again while its neighbours go on decoding.  A row decodes exactly what gsv_t2s_prefill_ragged + gsv_t2s_decode decode for it
 * with the same counter-RNG key (fp32: the same bits whatever the chunks and the neighbours are).
 *
 * begin: slots <= max_batch.  The scalars of sp (early_stop_num, eos_mask_steps, max_steps; top_k .. repetition_penalty unless
 *   row_sampling != 0) hold for the whole session; sp->seed is unused, every row brings its key.  out_tokens [dev] int32
 *   [slots][sp->max_steps] and out_len [dev] int32 [slots] stay the caller's and must outlive the session; slot b's entries are
 *   valid from the advance that reports it finished until the slot is admitted again.  Hooks set by gsv_t2s_set_debug before
 *   begin hold for the session, indexed by slot ([slots][max_steps], [max_steps][slots][vocab], [max_steps][slots][2]) and by
 *   the row's own step.  Sessions draw with the counter RNG only.  While a session is open gsv_t2s_prefill,
 *   gsv_t2s_prefill_ragged and gsv_t2s_decode return GSV_ERR_STATE and change nothing; a second begin is GSV_ERR_STATE too.
 * admit: prefills n rows (arguments as gsv_t2s_prefill_ragged, row i's key = (rng_seeds[i], rng_rows[i]) [host], its sampling
 *   tuple row_sampling[i] [host] if the session has per-row sampling, else NULL) and runs their step 0, then puts row i into
 *   slot_ids[i] [host].  No other slot is touched.  GSV_ERR_ARG before any launch: a slot that is live or out of range, a
 *   repeated slot, an RNG row outside [0, 2^24), a row with phone_lens + P_b + 2 + budget > max_seq, or P_b + budget beyond the position table or the token
 *   history (budget = min(max_steps, early_stop_num + 1)).
 * advance: at most n_steps further steps for every live slot; live_out / steps_out [host] int[slots] receive which slots are
 *   still live and every slot's step counter (either may be NULL).  fp16 on the v1/v2 shape with slots <= 128 runs the chunk as
 *   one launch of the persistent engine (a hand-off timeout re-runs the chunk on the launch-per-phase step), otherwise as
 *   n_steps replays of the step graph.  gsv_t2s_decode_info then describes this chunk.
 * release: takes the rows of the n named slots [host] out of the decode (a cancelled request): one small launch clears their
 *   live words, the next advance skips them and the slots can be admitted again.  A slot that holds no live row is left as it
 *   is; no other slot, and no K/V, is touched.  GSV_ERR_ARG before the launch: a slot out of range or given twice.
 * end: closes the session; the handle behaves as before. */
int gsv_t2s_session_begin(gsv_t2s_t* h, const gsv_sampling_params* sp, int slots, int row_sampling, int32_t* out_tokens,
                          int32_t* out_len);
int gsv_t2s_session_admit(gsv_t2s_t* h, int n, const int32_t* slot_ids, const int32_t* phones, const int32_t* phone_lens,
                          const float* bert, const int32_t* prompts_packed, const int32_t* prompt_lens, const uint64_t* rng_seeds,
                          const int32_t* rng_rows, const gsv_row_sampling_t* row_sampling, gsv_stream_t stream);
int gsv_t2s_session_advance(gsv_t2s_t* h, int n_steps, int* live_out, int* steps_out, gsv_stream_t stream);
int gsv_t2s_session_release(gsv_t2s_t* h, int n, const int32_t* slot_ids, gsv_stream_t stream);
int gsv_t2s_session_end(gsv_t2s_t* h);
/* test hook: the slots' row state, state [host] int32 [4][slots] = cached positions | live | step counter | prompt length;
 * waits for the device */
int gsv_t2s_session_state(gsv_t2s_t* h, int32_t* state);
/* measurement hook: HIP-event time (ms) of the last admission's adopt launch and the K/V bytes it read (it writes as many) */
int gsv_t2s_session_adopt_info(gsv_t2s_t* h, float* device_ms, int64_t* kv_bytes);

/* How the last gsv_t2s_decode call ran: mode 1 = the persistent engine (csrc/t2s_mega.hip: fp16, d=512/16 heads/FFN 2048,
 * B <= 128 -- up to four quads of rows per row group, B <= 32 is one quad; all steps after step 0 in ONE launch, hand-offs on the chip), mode 0 = one hipGraph of 122 launches per step
 * (fp32, other shapes, GSV_T2S_NO_MEGA=1, or a device on which the engine's 256 workgroups are not co-resident);
 * device_ms = HIP-event time of the persistent launch, steps = decode steps it covered (mode 1 only). */
int gsv_t2s_decode_info(gsv_t2s_t* h, int* mode, float* device_ms, int* steps);
/* A/B switch inside one process: on = 0 makes later decode calls of this handle use the launch-per-phase step */
int gsv_t2s_set_mega(gsv_t2s_t* h, int on);
/* A/B switch of the prefill's four per-layer GEMMs (fp16): mode 0 = the conv / GEMM dispatcher only, 1 = the panel kernel
 * (csrc/gemm_panel.hip) wherever it is eligible, whatever the row count, 2 (default) = the panel kernel from the measured row-count
 * threshold upwards.  Either way the prefill computes the same bits: the kernel takes the summation form of the kernel the
 * dispatcher would launch for the shape, and a GEMM for which it has no such form stays on the dispatcher.  GSV_NO_PREFILL_PANEL (set, read once per process) forces
 * mode 0 for every handle.  Another mode is GSV_ERR_ARG. */
int gsv_t2s_set_prefill_gemm(gsv_t2s_t* h, int mode);
/* Robustness report.  A persistent launch whose hand-off timed out (a member workgroup was not running: its CU was held
 * by another kernel) does not fail the request: the row state is restored, the batch is re-run on the launch-per-phase
 * step and the handle stops using the engine.  engine_available = 0 after that (or when the engine was never built),
 * fallbacks = launches that ended that way, last_error3 [host] = {epoch, workgroup, hop code} of the last timeout. */
int gsv_t2s_engine_stats(gsv_t2s_t* h, int* engine_available, int* fallbacks, unsigned* last_error3);
/* Parity hooks for the NEXT gsv_t2s_decode call only (both decode paths, every dtype; not a reference feature -- SURVEY.md
 * section 7 asks for a teacher-forced logit comparison of the fp16 engine):
 *   force_tokens [dev] int32 [B][max_steps] or NULL: step s of row b continues with force_tokens[b][s] instead of the
 *     token it sampled (EOS / early-stop bookkeeping then sees the forced token);
 *   logits_dump [dev] fp32 [max_steps][B][vocab] or NULL: raw logits (before the repetition penalty) of every step run;
 *   drawn_dump [dev] int32 [max_steps][B][2] or NULL: (token the sampler drew, argmax of the penalised logits) of every
 *     step run, recorded BEFORE forcing -- lets a test replay the engine's sampling (noise indexing, counter RNG, repetition
 *     bookkeeping) step by step with gsv_op_sample / the oracle on the dumped logits. */
int gsv_t2s_set_debug(gsv_t2s_t* h, const int32_t* force_tokens, float* logits_dump, int32_t* drawn_dump);
/* Per-token log-probabilities for the NEXT gsv_t2s_decode call only (like gsv_t2s_set_debug; NULL: none, the default).
 * out_logp [dev] fp32 [B][max_steps], indexed like out_tokens: entry [b][s] = x[t] - max(x[:Veff]) - log(sum_{v < Veff}
 * exp(x[v] - max)) with x the raw logits of row b at step s (what logits_dump records: temperature 1, no repetition penalty,
 * no top-k / top-p cut), Veff the step's unmasked vocabulary (EOS masked while s < eos_mask_steps) and t the token the row
 * takes: the sampled one, or the forced one under force_tokens (a token in the masked EOS column: -inf).  The step that ends
 * a row has its entry too, at [b][out_len[b]]; entries of steps a row never ran are left as the caller filled them.  Both
 * decode paths write it, and a persistent launch that falls back and re-runs on the launch path rewrites the same values.
 * Set before gsv_t2s_session_begin it holds for the session as [slots][max_steps], indexed by slot and the row's own step.
 * Sampling is not changed by it: the same tokens with and without. */
int gsv_t2s_set_logprobs(gsv_t2s_t* h, float* out_logp);
/* test hook: member `member` (0..31) of row group 0 skips ONE hand-off publish in the next persistent launch, which must then
 * end through its bounded waits (never hang), be re-run on the launch-per-phase step and be counted by gsv_t2s_engine_stats */
int gsv_t2s_debug_stall(gsv_t2s_t* h, int member);
/* test hook: logits of each row's last sampled step [dev] fp32 [B][vocab] (either decode path) */
int gsv_t2s_debug_logits(gsv_t2s_t* h, float* out, gsv_stream_t stream);
/* test hook: positions 0 .. n_pos - 1 of batch row `row` in one layer's K (which = 0) or V (which = 1) cache, copied to out
 * [host] [heads][n_pos][32] in the handle's dtype; waits for the device.  GSV_ERR_ARG: a layer, row or n_pos outside the arena. */
int gsv_t2s_debug_kv(gsv_t2s_t* h, int layer, int which, int row, int n_pos, void* out);
/* per-kernel timing of the decode step: average device time (ms) of one step over `iters`
 * replays at the current cache length, and of the decode-attention kernel alone. */
int gsv_t2s_time_step(gsv_t2s_t* h, int iters, float* step_ms, float* attn_ms, gsv_stream_t stream);
/* measurement hook: B rows with kv_len cached positions each (zeroed cache), for kernel timing sweeps */
int gsv_t2s_debug_set_state(gsv_t2s_t* h, int B, int kv_len);
/* algorithmic HBM bytes of one decode step at the current state */
int64_t gsv_t2s_step_bytes(gsv_t2s_t* h, int64_t* attn_bytes);

/* ---------------------------------------------------------------------------------------
 * SoVITS v2 waveform decoder (H6-H12)
 * ------------------------------------------------------------------------------------- */
typedef struct gsv_vits gsv_vits_t;

typedef struct {
  int inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size;
  int gin_channels, n_symbols, ssl_dim, n_bins, upsample_initial_channel;
  int n_ups;
  int up_rates[8];
  int up_kernels[8];
  int n_resblocks;          /* resblocks per stage (3) */
  int rb_kernels[4];
  int rb_dilations[4][3];
  int ref_bins;             /* 704 (v2): leading spectrogram bins fed to ref_enc */
  int flavor;               /* 0 = v1/v2 SynthesizerTrn (flow + generator); 1 = v3, 2 = v4 SynthesizerTrnV3 (bridge + wns1,
                               nearest x1.875 / x2; no flow / generator weights: the mel comes from gsv_cfm_inference) */
  int v2pro;                /* 1 = v2Pro / v2ProPlus conditioning (module/models.py:895-899): sv_emb 20480 -> gin, PReLU(gin),
                               ge_to512 for the MRTE; gin_channels may then differ from 512 */
} gsv_vits_config;

int gsv_vits_create(const gsv_vits_config* cfg, int dtype, gsv_vits_t** out);
void gsv_vits_destroy(gsv_vits_t* h);
int gsv_vits_load_tensor(gsv_vits_t* h, const char* name, const float* data, int64_t numel);
int gsv_vits_finalize(gsv_vits_t* h); /* folds weight-norm, repacks conv weights */

/* ge = mean over references of ref_enc(spec[:ref_bins]) (models.py:962-984).  specs [host] array
 * of n_refs [dev] fp32 pointers, each [bins][frames[i]] channels-first as the reference holds it. */
int gsv_vits_set_refer(gsv_vits_t* h, const float* const* specs, const int* frames, int bins, int n_refs,
                       gsv_stream_t stream);
/* codes [dev] int32 [T], phones [dev] int32 [L]; frames F = 2T when speed == 1, else int(2T/speed)+1
 * (linear interpolation of the encoder output, models.py:226-228); noise [dev] fp32 [inter][F]
 * channels-first (the randn_like draw of models.py:1000; NULL = counter RNG keyed by seed),
 * wav [dev] fp32 [F * prod(up_rates)]. */
int gsv_vits_decode(gsv_vits_t* h, const int32_t* codes, int T, const int32_t* phones, int L, const float* noise,
                    float noise_scale, double speed, uint64_t seed, float* wav, gsv_stream_t stream);
/* ssl [dev] fp32 [ssl_dim][T50] channels-first -> codes [dev] int32 [T50/2] */
int gsv_vits_extract_latent(gsv_vits_t* h, const float* ssl, int T50, int32_t* codes, gsv_stream_t stream);
/* test hook: copy a named intermediate of the last decode ("ge","m_p","logs_p","z", "gen_last_in" = the last generator stage's input)
 * into out [dev] fp32 in channels-first [C][T] order; returns element count via *numel. */
int gsv_vits_debug_tensor(gsv_vits_t* h, const char* name, float* out, int64_t cap, int64_t* numel,
                          gsv_stream_t stream);
/* the same for the MRTE attention's operands of the last enc_p: "m_q" [512][2T] and "m_kv" [1024][L] (keys = channels 0..511);
 * after a segmented decode, the padded rows of its layout. */
/* Phoneme alignment (csrc/align.hip, gsv_op_align below): spans [host] [n], each a run of codes and a run of phones of one
 * segment in the segment's own packed indices (segment = 0 for gsv_vits_decode / _decode_encp); its frames are
 * 2 * code0 .. 2 * (code0 + n_codes) of the 50-per-second pre-speed axis.  The table is pending for the NEXT gsv_vits_decode /
 * gsv_vits_decode_segments[_speed] / gsv_vits_decode_encp on the handle and consumed by it: that call issues the two alignment
 * launches on its stream right after the MRTE attention, on the attention's own q and k, and writes ends [dev] int32
 * [sum n_phones] (span r's phonemes after those of the spans in front of it; frames counted from the span's first frame) and
 * score [dev] fp32 [n].  A span outside its segment, or two spans that share a phoneme, make that call fail with GSV_ERR_ARG
 * before it launches anything.  NULL spans or n = 0 clears a pending table.  Without a pending table a decode issues exactly
 * the launches it issued before, and a pending table changes no value the decode computes. */
typedef struct gsv_align_seg_span {
  int32_t segment, code0, n_codes, phone0, n_phones;
} gsv_align_seg_span_t;
int gsv_vits_set_align(gsv_vits_t* h, const gsv_align_seg_span_t* spans, int n, int32_t* ends, float* score);
/* v3 / v4 (H14, SynthesizerTrnV3.decode_encp, module/models.py:1243-1267): codes / phones as in gsv_vits_decode ->
 * fea [dev] fp32 [512][F] (channels-first, what the reference returns; ge comes from gsv_vits_set_refer).
 * F = gsv_vits_encp_frames(h, T, speed) = floor(frames_after_speed * (1.875 | 2)); returns -1 on bad arguments. */
int gsv_vits_encp_frames(gsv_vits_t* h, int T, double speed);
int gsv_vits_decode_encp(gsv_vits_t* h, const int32_t* codes, int T, const int32_t* phones, int L, double speed, float* fea,
                         gsv_stream_t stream);
/* v2Pro / v2ProPlus (N4, module/models.py:971-975): as gsv_vits_set_refer, plus one speaker-verification embedding per
 * reference (sv_embs [host] array of n_refs [dev] fp32 pointers to 20480 values): ge_r = PReLU(ref_enc(spec_r) + sv_emb(sv_r)),
 * ge = mean_r ge_r; the MRTE receives ge_to512(ge). */
int gsv_vits_set_refer_sv(gsv_vits_t* h, const float* const* specs, const int* frames, int bins, const float* const* sv_embs,
                          int n_refs, gsv_stream_t stream);
/* Segmented decode (v1 / v2 / v2Pro / v2ProPlus): n independent sequences, each with its own voice and seed, in one
 * pass of enc_p, flow and generator.  The library lays the segments back to back with G zero "gap" frames between them
 * (G = gsv_vits_segment_gap(cfg), G * prod(up_rates[:i]) rows after upsampling stage i, G rows between phone runs); every
 * tensor a conv reads keeps its gap rows at 0 and attention is block-diagonal, so segment s yields what gsv_vits_decode of
 * segment s alone yields.
 * gsv_vits_store_voice copies the conditioning of the last gsv_vits_set_refer / _set_refer_sv into voice slot `slot`
 * (0 <= slot < GSV_VITS_MAX_VOICES).  gsv_vits_decode_segments: codes [dev] int32 [sum code_lens], phones [dev] int32
 * [sum phone_lens], both packed without gaps; code_lens / phone_lens / voice_slots / seeds [host] [n]; noise [dev] fp32
 * [inter][sum 2 code_lens] or NULL (segment s draws the counter RNG keyed by seeds[s]); wav [dev] fp32, segment s's
 * 2 * code_lens[s] * prod(up_rates) samples back to back.
 * gsv_vits_decode_segments_speed: the same with speeds [host] [n] (each finite and > 0; NULL = all 1, which is
 * gsv_vits_decode_segments).  Two layouts share the gap G and the phone axis: the pre layout (2 * code_lens[s] frames per
 * segment: codebook gather, enc_ssl, MRTE, enc2) and the post layout (F_s frames: proj, flow, generator, wav), F_s =
 * 2 * code_lens[s] at speed 1, else (int)(2 * code_lens[s] / speeds[s]) + 1 as in gsv_vits_decode.  One kernel interpolates
 * each segment from its own pre rows into its post rows (gap rows written as zeros); when no segment changes its frame count
 * the post layout is the pre layout and nothing extra runs.  noise is [inter][sum F_s], wav holds segment s's
 * F_s * prod(up_rates) samples back to back; segment s yields what gsv_vits_decode(speed = speeds[s], seed = seeds[s]) yields.
 * A speed that is not finite or <= 0, or a layout of 2^24 rows or more, is an error code. */
#define GSV_VITS_MAX_VOICES 128
int gsv_vits_store_voice(gsv_vits_t* h, int slot);
int gsv_vits_decode_segments(gsv_vits_t* h, int n, const int32_t* codes, const int* code_lens, const int32_t* phones,
                             const int* phone_lens, const int* voice_slots, const uint64_t* seeds, const float* noise,
                             float noise_scale, float* wav, gsv_stream_t stream);
int gsv_vits_decode_segments_speed(gsv_vits_t* h, int n, const int32_t* codes, const int* code_lens, const int32_t* phones,
                                   const int* phone_lens, const int* voice_slots, const uint64_t* seeds, const double* speeds,
                                   const float* noise, float noise_scale, float* wav, gsv_stream_t stream);
/* host-only planning helpers (no device needed): the gap G in frames, and the segment id (-1 = gap) of every row at `level`
 * (-1 = phones, 0 = frames, i = after upsampling stage i); *rows = row count (seg may be NULL to query it).
 * gsv_vits_segment_map_speed is the map of the post layout of gsv_vits_decode_segments_speed (level >= 0: frames after the
 * speed interpolation x the upsampling so far; level -1: phones, unchanged). */
int gsv_vits_segment_gap(const gsv_vits_config* cfg);
int gsv_vits_segment_map(const gsv_vits_config* cfg, int n, const int* code_lens, const int* phone_lens, int level, int32_t* seg,
                         int64_t cap, int64_t* rows);
int gsv_vits_segment_map_speed(const gsv_vits_config* cfg, int n, const int* code_lens, const int* phone_lens, const double* speeds,
                               int level, int32_t* seg, int64_t cap, int64_t* rows);
/* per-kernel timing hooks for bench.py: device ms of the last decode's generator section */
int gsv_vits_last_timing(gsv_vits_t* h, float* total_ms, float* generator_ms);

/* ---------------------------------------------------------------------------------------
 * v3 / v4 vocoders (H15, H16): mel [in_channels][F] -> waveform.
 *   kind 0 = HiFi-GAN `Generator` as used for v4 (TTS_infer_pack/TTS.py:631-648, module/models.py:407-471:
 *            leaky-relu 0.1, conv_post bias, tanh); kind 1 = BigVGAN-v2 (BigVGAN/bigvgan.py:226-355:
 *            AMPBlock1 with anti-aliased Snake/SnakeBeta, clamp or tanh at the end).
 * Tensor names = the reference state-dict keys (weight-norm pairs or folded weights both accepted).
 * ------------------------------------------------------------------------------------- */
typedef struct gsv_vocoder gsv_vocoder_t;

typedef struct {
  int kind;
  int in_channels;               /* 100 mel bands */
  int upsample_initial_channel;
  int n_ups;
  int up_rates[8];
  int up_kernels[8];
  int n_resblocks;
  int rb_kernels[4];
  int rb_dilations[4][3];
  int bias_at_final;             /* conv_post bias */
  int tanh_at_final;             /* else clamp to [-1, 1] */
  int snake_logscale;            /* BigVGAN: alpha/beta stored in log scale */
} gsv_vocoder_config;

int gsv_vocoder_create(const gsv_vocoder_config* cfg, int dtype, gsv_vocoder_t** out);
void gsv_vocoder_destroy(gsv_vocoder_t* h);
int gsv_vocoder_load_tensor(gsv_vocoder_t* h, const char* name, const float* data, int64_t numel);
int gsv_vocoder_finalize(gsv_vocoder_t* h);
/* mel [dev] fp32 [in_channels][F] channels-first (as the reference passes it), wav [dev] fp32 [F * prod(up_rates)] */
int gsv_vocoder_forward(gsv_vocoder_t* h, const float* mel, int F, float* wav, gsv_stream_t stream);
/* Segmented pass: n independent mels (e.g. one per voice) through ONE pass of the generator.  The library lays the segments
 * back to back with G zero "gap" frames between neighbours (G = gsv_vocoder_segment_gap(cfg), G * prod(up_rates[:i]) rows after
 * upsampling stage i).  Every tensor a conv reads keeps its gap rows at 0, and BigVGAN's anti-aliased activation replicates
 * each segment's own edge rows at both rates and never reads a gap row, so segment s yields what gsv_vocoder_forward of
 * segment s alone yields.  mel [dev] fp32 [in_channels][sum frames], the segments packed without gaps; frames [host] [n];
 * wav [dev] fp32 [sum frames * prod(up_rates)], segment s's samples back to back.  n == 1 is gsv_vocoder_forward itself.
 * Errors before anything is launched: a null argument, n < 1 or n > 4096, a frames[s] < 1, a gapped layout of 2^24 rows or
 * more at the output rate. */
int gsv_vocoder_forward_segments(gsv_vocoder_t* h, const float* mel, int n, const int* frames, float* wav, gsv_stream_t stream);
/* host-only planning helpers (no device needed), the counterparts of gsv_vits_segment_gap / gsv_vits_segment_map: the gap G in
 * frames (-1 for a bad config), taken from the generator's shape by the rule of the SoVITS segmented decode (conv_pre, the
 * transposed ups, every ResBlock conv at its resolution, conv_post), and the segment id (-1 = gap) of every row at `level`
 * (0 = mel frames, i = after upsampling stage i): (sum frames + (n - 1) G) * prod(up_rates[:level]) rows into seg [cap]. */
int gsv_vocoder_segment_gap(const gsv_vocoder_config* cfg);
int gsv_vocoder_segment_map(const gsv_vocoder_config* cfg, int n, const int* frames, int level, int32_t* seg, int64_t cap);

/* ---------------------------------------------------------------------------------------
 * v3 / v4 flow-matching mel decoder (H14): CFM.inference (module/models.py:1027-1085) over the DiT estimator
 * (f5_tts/model/backbones/dit.py:88-194).  gsv_cfm_inference and gsv_cfm_inference_rows are inference_cfg_rate = 0, as
 * every caller in the reference passes it; gsv_cfm_inference_guided takes the rate (classifier-free guidance).
 * Tensor names = the DiT state-dict keys (the part after "cfm.estimator." in a v3/v4 SoVITS checkpoint).
 * The rotary embedding follows x_transformers' published definition (un-vendored dependency: parity unpinned).
 * ------------------------------------------------------------------------------------- */
typedef struct gsv_cfm gsv_cfm_t;

typedef struct {
  int dim, depth, heads, dim_head, ff_mult;   /* 1024, 22, 16, 64, 2 (module/models.py:1219-1222) */
  int mel_dim, text_dim, conv_layers;         /* 100, 512, 4 */
} gsv_dit_config;

int gsv_cfm_create(const gsv_dit_config* cfg, int dtype, gsv_cfm_t** out);
void gsv_cfm_destroy(gsv_cfm_t* h);
int gsv_cfm_load_tensor(gsv_cfm_t* h, const char* name, const float* data, int64_t numel);
int gsv_cfm_finalize(gsv_cfm_t* h);
/* mu [dev] fp32 [B][T][text_dim] (the `fea` tensor as CFM.inference receives it), prompt [dev] fp32 [B][mel_dim][Tp]
 * (the reference mel, frames >= Tp are generated), noise [dev] fp32 [B][mel_dim][T] = the randn draw of models.py:1030,
 * or NULL to draw it on the device from `seed`; out [dev] fp32 [B][mel_dim][T] (prompt frames are zero, as in the
 * reference).  n_steps Euler steps with d = 1/n_steps. */
int gsv_cfm_inference(gsv_cfm_t* h, const float* mu, const float* prompt, int B, int T, int Tp, int n_steps,
                      const float* noise, float temperature, uint64_t seed, float* out, gsv_stream_t stream);
/* The same over B rows that each have their own prompt: prompts [host] B device pointers, row b's fp32 [mel_dim][Tp[b]]
 * (may be NULL where Tp[b] == 0), Tp [host] B lengths, 0 <= Tp[b] <= T; seeds [host] B noise keys, used where noise is NULL
 * (one of the two must be given).  Row b draws what gsv_cfm_inference draws for a row whose seed + 0x9E3779B97F4A7C15 * b
 * equals seeds[b]: no offset is added here.  out [dev] fp32 [B][mel_dim][T], row b's first Tp[b] frames zero.  A bad
 * argument returns an error before anything is launched. */
int gsv_cfm_inference_rows(gsv_cfm_t* h, const float* mu, const float* const* prompts, const int* Tp, int B, int T,
                           int n_steps, const float* noise, const uint64_t* seeds, float temperature, float* out,
                           gsv_stream_t stream);
/* gsv_cfm_inference_rows with classifier-free guidance (models.py:1063-1081): arguments, noise keys and output as there.
 * cfg_rate > 1e-5 (the reference's own test) runs every row twice per Euler step inside ONE DiT pass over 2 B rows -- as
 * given, and with the prompt columns and the text zeroed (the text before its positional table and ConvNeXt stack) -- and
 * steps with v + (v - v_uncond) * cfg_rate.  cfg_rate <= 1e-5, negative rates included, is gsv_cfm_inference_rows itself.
 * cfg_rate must be finite and 2 * B <= 65535 when guided; both are checked before anything is launched. */
int gsv_cfm_inference_guided(gsv_cfm_t* h, const float* mu, const float* const* prompts, const int* Tp, int B, int T,
                             int n_steps, const float* noise, const uint64_t* seeds, float temperature, float cfg_rate,
                             float* out, gsv_stream_t stream);

/* LoRA adapters (fine-tuned v3 / v4 voices, reference s2_train_v3_lora.py:134-139: rank-r adapters on to_q / to_k / to_v /
 * to_out.0 of every DiT block) held beside the base weights, so rows of ONE pass may each use their own voice.  An adapter is
 * staged like the base weights: begin (rank 1 .. GSV_LORA_MAX_RANK, alpha > 0; the reference trains with alpha = rank), one
 * load_tensor per matrix -- names transformer_blocks.<i>.attn.{to_q,to_k,to_v,to_out.0}.lora_{A,B}, host fp32, lora_A
 * [rank][in], lora_B [out][rank] -- then finalize, which checks that all 4 * depth pairs are there with the right sizes and
 * nothing else, uploads them (engine dtype, rank padded to a multiple of 16, alpha / rank folded into lora_B in fp32) and
 * returns the slot: a small integer, reused after gsv_cfm_adapter_remove, at most GSV_CFM_MAX_ADAPTERS live at once.  A
 * failed finalize drops the staged tensors and leaves the store as it was.  None of these may run while a pass of the same
 * handle is in flight. */
#define GSV_CFM_MAX_ADAPTERS 256
#define GSV_LORA_MAX_RANK 128
int gsv_cfm_adapter_begin(gsv_cfm_t* h, int rank, float alpha);
int gsv_cfm_adapter_load_tensor(gsv_cfm_t* h, const char* name, const float* data, int64_t numel);
int gsv_cfm_adapter_finalize(gsv_cfm_t* h, int* slot);
int gsv_cfm_adapter_remove(gsv_cfm_t* h, int slot);   /* an error while a live row of an open session uses the slot */
int gsv_cfm_adapter_count(gsv_cfm_t* h);   /* live adapters, or a negative error code */
/* gsv_cfm_inference_guided (cfg_rate <= 1e-5: gsv_cfm_inference_rows) whose row b runs the DiT with adapter adapters[b]
 * ([host] B slots; -1 = the base model; NULL = every row the base model): after the q/k/v GEMM and after the out-projection
 * GEMM of every block the rows with a slot receive (alpha / r) * B A x, under the out-projection's gate.  A guided row's
 * unconditioned twin takes the row's slot.  A pass without an adapted row issues exactly the launches of the entry above.
 * A slot that is out of range or not live returns an error before anything is launched. */
int gsv_cfm_inference_adapted(gsv_cfm_t* h, const float* mu, const float* const* prompts, const int* Tp, const int* adapters,
                              int B, int T, int n_steps, const float* noise, const uint64_t* seeds, float temperature,
                              float cfg_rate, float* out, gsv_stream_t stream);

/* Flow-matching sessions (csrc/cfm_session.hip): a pass whose rows carry their own time -- their own step count, step index,
 * guidance rate and LoRA slot -- and enter and leave between Euler steps.  One session per handle, rows of T frames.
 * rows_cap (1 .. GSV_CFM_SESSION_MAX_ROWS) is the number of slots and the cap on live DiT rows; a guided row (cfg_rate > 1e-5)
 * counts 2, it brings its unconditioned twin.  While a session is open the one-shot entries above return an error.
 * The session issues nothing on its own: every launch happens inside the call that asks for it, on that call's stream;
 * the calls of one session must be ordered (one stream, or the caller's own events).
 *
 * admit: n rows into the free slots `slots` ([host] n distinct ints): mu [dev] fp32 [n][T][text_dim], prompts / Tp / adapters
 *   ([host], adapters NULL = the base model) as gsv_cfm_inference_adapted, n_steps ([host] n ints, each 1 .. 1024) and cfg_rate
 *   ([host] n floats) per row, noise [dev] fp32 [n][mel_dim][T] or NULL and seeds ([host] n keys) as gsv_cfm_inference_rows.
 *   Runs the text stack and the noise draw of these rows and keeps the results (and a copy of the prompt frames) in the slots:
 *   nothing of the caller's is read once the call's launches have run.  Refused, before anything is launched: an occupied or
 *   repeated slot, live DiT rows + new ones above rows_cap, n_steps outside [1, 1024], Tp > T, a null prompt with Tp > 0, an
 *   adapter that is not live, more than 8 distinct step counts among the live rows (the modulation tables are cached per
 *   step count on the handle, at most 8 tables and 1 GiB, least recently used dropped first; a new step count costs one
 *   stream synchronisation).
 * step: k Euler steps of every live row; a row that has taken its n_steps steps is finished and takes no part in later
 *   steps of the same call.  Row b at its step i uses exactly the modulations and the d of step i of a one-shot call with
 *   n_steps_b steps.  The DiT of one step runs over the live rows in ascending slot order, then the twins of the guided ones in
 *   the same order; free and finished slots cost nothing.  Returns at once when no row is live.
 * fetch: a finished row as out [dev] fp32 [mel_dim][T], its prompt frames zero; frees the slot.  A live or free slot is an error.
 * fetch_mel: n finished rows (slots [host] n distinct ints, 1 <= n <= rows_cap) in ONE launch, straight into the layout the
 *   vocoder reads: entry i writes the generated frames t in [Tp_i, T) of slot slots[i] -- Tp_i the prompt length recorded at
 *   admission -- de-normalised, ((x + 1) / 2) * (hi - lo) + lo in that order and uncontracted, channels-first, to columns
 *   [col0[i], col0[i] + T - Tp_i) of out [dev] fp32 [mel_dim][ld] (col0 [host] n ints).  The bits are those of
 *   denorm_spec(fetch(slot)[:, Tp_i:]).  The [T][mel] -> [mel][T] transpose goes through an LDS tile, so a wave reads and writes
 *   contiguously.  Frees the slots, as fetch does.  Refused, before anything is launched and with every slot left as it was: a
 *   slot that is not finished, a repeated slot, n outside [1, rows_cap], a null pointer, col0[i] < 0, col0[i] + T - Tp_i > ld.
 *   The destination ranges are NOT checked against each other: entries whose column ranges overlap race, the caller keeps them apart.
 * release: drops live or finished rows; the others are not touched.
 * gsv_cfm_adapter_remove refuses a slot that a live row of the open session still runs with.
 * state: [host] int32 [3][rows_cap] = 0 free / 1 live / 2 finished | steps taken | n_steps.  Host bookkeeping, no device wait.
 * end: closes the session (rows still in it are dropped); the one-shot entries work again. */
#define GSV_CFM_SESSION_MAX_ROWS 64
int gsv_cfm_session_begin(gsv_cfm_t* h, int rows_cap, int T, float temperature, gsv_stream_t stream);
int gsv_cfm_session_admit(gsv_cfm_t* h, int n, const int32_t* slots, const float* mu, const float* const* prompts, const int* Tp,
                          const int* adapters, const int* n_steps, const float* cfg_rate, const float* noise,
                          const uint64_t* seeds, gsv_stream_t stream);
int gsv_cfm_session_step(gsv_cfm_t* h, int k, gsv_stream_t stream);
int gsv_cfm_session_fetch(gsv_cfm_t* h, int slot, float* out, gsv_stream_t stream);
int gsv_cfm_session_fetch_mel(gsv_cfm_t* h, int n, const int32_t* slots, const int* col0, long long ld, float lo, float hi,
                              float* out, gsv_stream_t stream);
int gsv_cfm_session_release(gsv_cfm_t* h, int n, const int32_t* slots);
int gsv_cfm_session_state(gsv_cfm_t* h, int32_t* state);
int gsv_cfm_session_end(gsv_cfm_t* h);

/* ---------------------------------------------------------------------------------------
 * SOLA stitching of the chunked v3/v4 vocoder output (H17, TTS.sola_algorithm, TTS_infer_pack/TTS.py:1611-1637).
 * frags [dev] fp32: the n fragments back to back (lens [host] samples each, every one >= 2 * overlap); modified in
 * place (cross-faded heads).  out [dev] fp32, capacity sum(lens); *out_len [host] = stitched length.  Synchronises
 * the stream (the length depends on the argmax offsets found on the device).
 * ------------------------------------------------------------------------------------- */
int gsv_sola(float* frags, const int* lens, int n, int overlap, float* out, int* out_len, gsv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * H13 audio post-processing (replaces TTS.audio_postprocess, TTS_infer_pack/TTS.py:1377-1429): per fragment divide by
 * its peak when the peak exceeds 1, append `gap` zero samples, concatenate in the order given, scale by 32768 in the
 * fragments' dtype and truncate to int16 (numpy's astype wrap).  frags [host] n device pointers (output order),
 * lens [host] n sample counts, out [dev] int16 with capacity sum(lens) + n * gap.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------- */
int gsv_postprocess(const void* const* frags, const int* lens, int n, int dtype, int gap, int16_t* out, gsv_stream_t stream);
/* the same fragments, peak rule, gaps and order, written as fp32 without the x32768 / int16 step (out capacity as above): the
 * float concatenation the reference's super-sampling path feeds to AP_BWE (TTS.py:1397-1417) */
int gsv_postprocess_f32(const void* const* frags, const int* lens, int n, int dtype, int gap, float* out, gsv_stream_t stream);
/* gsv_postprocess for the fragments of several requests at once: n sentences (frags, lens [host], as above) in n_groups groups,
 * group g the next group_n[g] sentences with its own gap group_gap[g] (both [host]).  out [dev] int16 is one packed buffer:
 * group g starts at sample group_off[g] ([host], n_groups + 1 entries, written by the call; the last one is the total, which is
 * the capacity out needs: sum over the sentences of len + their group's gap) and holds exactly what gsv_postprocess writes for
 * that group alone.  Sentences are cut into tiles over the whole GPU (two launches: peaks, then conversion), and any number of
 * sentences is taken.  table [host] and workspace [dev]: gsv_postprocess_groups_workspace(lens, n) bytes each (-1: a negative
 * length); the call fills `table`, uploads it to `workspace` with one copy on `stream` and allocates nothing.  `table` must stay
 * untouched until the stream has passed that copy (page-locked memory keeps the call asynchronous).  n = 0 is GSV_OK and
 * touches neither. */
long long gsv_postprocess_groups_workspace(const int* lens, int n);
int gsv_postprocess_groups(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                           int n_groups, int16_t* out, long long* group_off, void* table, void* workspace, gsv_stream_t stream);
/* gsv_postprocess_groups at another sample rate and in another encoding.  Per group g with sentences
 * x_0 .. x_{k-1} and gap G:
 *   stream    X_g = concat_i [norm(x_i), G zeros], N_g = sum(len_i + G) samples: what gsv_postprocess_f32 writes for that group
 *             alone (the peak rule, with the division in the fragments' dtype), never materialised;
 *   resample  Y_g[i] = sum_j h[i * down + half - j * up] * X_g[j],  j in [0, N_g) with the filter index in [0, h_len),
 *             h_len = 2 * half + 1, i in [0, m_g), m_g = ceil(N_g * up / down): the arithmetic of gsv_op_resample_poly_seg (one fp32
 *             accumulator per output, fmaf over its taps in ascending j), zeros beyond the group's ends, so an output's bits
 *             depend on its own group's samples alone;
 *   format    GSV_OUT_S16: y * 32768 in fp32, clamped to [-32768, 32767] and truncated toward zero (a resampled signal overshoots
 *             its input's peak, so this path saturates instead of wrapping); GSV_OUT_MULAW / GSV_OUT_ALAW: ITU-T G.711 of that
 *             int16, one byte per sample (the bytes of Python's audioop.lin2ulaw / lin2alaw at width 2); GSV_OUT_F32: y.
 * h [dev] fp32: the filter, as gsv.audio_io.resample_filter designs it; up = down = 1 with h = {1.0f} applies an encoding at the
 * model's own rate.  out [dev]: one packed buffer of int16, bytes or floats; group g starts at output sample group_off[g]
 * ([host], n_groups + 1 entries, written by the call; the last one is the capacity out needs).  A group without sentences writes
 * nothing; outputs whose taps touch a NaN are unspecified.  table [host] and workspace [dev]:
 * gsv_postprocess_groups_rate_workspace(lens, n, n_groups) bytes each (-1: a negative length or count); filled, uploaded and kept
 * as for gsv_postprocess_groups, nothing is allocated.  Two launches: the peaks (the kernel of gsv_postprocess_groups), then one
 * workgroup per 1024 consecutive outputs of a group.  Refused with a message: an even h_len, one above 65535, and a pair whose
 * input window per 1024 outputs, (1023 * down + h_len - 1) / up + 2 samples, exceeds 16384. */
#define GSV_OUT_S16 0
#define GSV_OUT_MULAW 1
#define GSV_OUT_ALAW 2
#define GSV_OUT_F32 3
long long gsv_postprocess_groups_rate_workspace(const int* lens, int n, int n_groups);
int gsv_postprocess_groups_rate(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                                int n_groups, void* out, long long* group_off, void* table, void* workspace, const float* h,
                                int h_len, int up, int down, int out_fmt, gsv_stream_t stream);
/* gsv_postprocess_groups_rate with loudness normalisation after ITU-R BS.1770, measured and applied on
 * the device.  A span is a run of consecutive sentences of one group that is metered on its own and gets one gain:
 *   samples   gaps = 1: concat_i [norm(x_i), G zeros] over its sentences (the whole X_g when it names all of a group);
 *             gaps = 0: concat_i norm(x_i); N samples at the model's rate `rate`, never materialised;
 *   weighting the two BS.1770 biquads re-derived for `rate` from the analogue prototype (shelf f0 = 1681.974450955533 Hz,
 *             G = 3.999843853973347 dB, Q = 0.7071752369554196; high-pass f0 = 38.13547087602444 Hz, Q = 0.5003270373238773, as
 *             libebur128 and pyloudnorm do), zero state at the span's start, fp64;
 *   blocks    s = round(0.1 * rate); e_j = sum of y^2 over sub-block j < J = floor(N / s); z_b = (e_b + .. + e_{b+3}) / (4 s),
 *             b <= J - 4; the trailing partial sub-block is ignored.  J < 4 and N > 0: the single block z_0 = sum of all y^2 / N;
 *   gating    l(z) = -0.691 + 10 log10 z; blocks with l > -70, then those of them with l > l(their mean) - 10; L = l(mean of
 *             those), -inf when none is left;
 *   gain      1 when target is NaN (meter only), L = -inf or a sentence of the span holds a NaN; else 10^((target - L) / 20),
 *             lowered to c / P with GSV_LOUD_LIMITED set when it would lift the span's peak P = max_i min(peak_i, 1) above
 *             c = 10^(peak_db / 20); fp64, rounded to fp32 once.
 * The gain multiplies the fp32 sample of the stream in front of the filter taps; resampling and formats are those of
 * gsv_postprocess_groups_rate.  Sentences in no span keep gain 1.  spans [host]: sorted by `first`, not overlapping, none across
 * two groups, -70 <= target <= 0 or NaN, peak_db <= 0, rate > 0: anything else is refused with a message before any launch, and
 * so is a rate whose sub-block s is not longer than 2048 samples (a 4096-sample tile of the meter touches at most three).
 * report [dev]: one record per span.  With n_spans = 0 the call is gsv_postprocess_groups_rate, launch for launch.  Otherwise
 * six launches whatever n, n_groups and n_spans: peaks, tile end states, carries, sub-block energies, gates, write.  No floating-
 * point atomics and no workgroup waits for another: a span's report and output bytes are bit-identical whatever else the call
 * holds.  table [host] and workspace [dev]: gsv_postprocess_groups_loud_workspace(...) bytes each (-1: a bad length, count or
 * rate); nothing is allocated and the host is not synchronised. */
typedef struct gsv_loud_span {
  int32_t first, count; /* sentences [first, first + count) of the call, all of one group */
  int32_t gaps;         /* 1: each sentence is followed by its group's gap; 0: the sentences alone */
  float target;         /* LUFS; NaN: meter only */
  float peak_db;        /* ceiling of the span's peak after the gain, dBFS <= 0 */
} gsv_loud_span;
typedef struct gsv_loud_report {
  double lufs; /* L; -inf when no block passes the gates; unspecified with GSV_LOUD_NAN */
  float gain;  /* the linear gain that was (gsv_op_loudness: would be) applied */
  uint32_t flags;
} gsv_loud_report;
#define GSV_LOUD_LIMITED 1u /* the ceiling lowered the gain */
#define GSV_LOUD_NAN 2u     /* a sentence of the span holds a NaN: gain 1 */
#define GSV_LOUD_SILENT 4u  /* L = -inf: gain 1 */
long long gsv_postprocess_groups_loud_workspace(const int* lens, int n, const int* group_n, const int* group_gap, int n_groups,
                                                int rate, int n_spans);
int gsv_postprocess_groups_loud(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                                int n_groups, void* out, long long* group_off, void* table, void* workspace, const float* h,
                                int h_len, int up, int down, int out_fmt, int rate, const gsv_loud_span* spans, int n_spans,
                                gsv_loud_report* report, gsv_stream_t stream);
/* test / debug: the meter of gsv_postprocess_groups_loud alone (its first five launches).  energies [dev] fp64: span k's
 * sub-block energies e_j at energy_off[k] .. energy_off[k + 1] ([host], n_spans + 1 entries, written by the call):
 * ceil(N_k / s) values, the last one the trailing partial sub-block where s does not divide N_k.  energies holds at most
 * sum over the groups of N_g / s, plus n_spans, values.  table, workspace: as above. */
int gsv_op_loudness(const void* const* frags, const int* lens, int n, int dtype, const int* group_n, const int* group_gap,
                    int n_groups, int rate, const gsv_loud_span* spans, int n_spans, double* energies, long long* energy_off,
                    gsv_loud_report* report, void* table, void* workspace, gsv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * AP-BWE audio super-resolution (tools/audio_sr.py::AP_BWE.__call__): torchaudio resample to hr_sampling_rate
 * (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99; restated from its published definition, parity unpinned against the
 * package itself), amp_pha_stft (AP_BWE_main/datasets1/dataset.py:9-27), APNet_BWE_Model.forward
 * (AP_BWE_main/models/model.py:76-147), amp_pha_istft (dataset.py:30-37).  Every shape value comes from the checkpoint's
 * config.json.  Tensor names = the reference state-dict keys (the "generator" dict), plus the two DFT bases the caller builds
 * (gsv/module/mel_processing.py::_dft_basis): "dft.forward" fp32 [n_fft/2+1 re rows | n_fft/2+1 im rows][n_fft] (periodic Hann
 * of win_size centred in n_fft) and "dft.inverse" fp32 [n_fft][n_fft/2+1 re | n_fft/2+1 im columns] (irfft / n_fft times the
 * window; the imaginary parts of the DC and Nyquist bins ignored).
 * ------------------------------------------------------------------------------------- */
typedef struct gsv_bwe gsv_bwe_t;

typedef struct {
  int n_fft, hop_size, win_size;    /* 1024, 80, 320 (assumed 24k -> 48k release) */
  int channels, layers;             /* ConvNeXt_channels 512, ConvNeXt_layers 8 */
  int hr_sampling_rate;             /* 48000 */
} gsv_bwe_config;

int gsv_bwe_create(const gsv_bwe_config* cfg, int dtype, gsv_bwe_t** out);
void gsv_bwe_destroy(gsv_bwe_t* h);
int gsv_bwe_load_tensor(gsv_bwe_t* h, const char* name, const float* data, int64_t numel);
int gsv_bwe_finalize(gsv_bwe_t* h);
/* output samples of a forward over n input samples at orig_sr: hop * floor(n_new / hop), n_new = ceil(n * hr / orig_sr)
 * (torch.istft with center=True and no length); -1 when the input is too short to reflect-pad by n_fft / 2 */
int gsv_bwe_out_len(gsv_bwe_t* h, int n, int orig_sr);
/* wav [dev] [n] of dtype (GSV_F16 / GSV_F32) at orig_sr -> out [dev] fp32 [gsv_bwe_out_len(h, n, orig_sr)] at hr_sampling_rate.
 * The workspace grows on demand; GSV_ERR_ARG when the resampled input has n_fft / 2 samples or fewer. */
int gsv_bwe_forward(gsv_bwe_t* h, const void* wav, int n, int dtype, int orig_sr, float* out, gsv_stream_t stream);
/* test hook: a stage of the last forward into out [dev] fp32: "resampled" [n_new], "log_amp", "pha", "mag_wb", "pha_wb"
 * channels-first [n_fft/2+1][frames] (the reference's [1, bins, T] tensors); element count via *numel */
int gsv_bwe_debug_tensor(gsv_bwe_t* h, const char* name, float* out, int64_t cap, int64_t* numel, gsv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * BigVGAN anti-aliased snake activation (v3 vocoder), the reference's one native kernel.
 * x,y [dev] [B][C][T] of `dtype`; up12/dn12 [dev] 12 filter taps; log_alpha/log_beta [dev] [C].
 * T == 0 returns GSV_OK without a launch (anti_alias_activation_cuda.cu:193-196).
 * ------------------------------------------------------------------------------------- */
int gsv_aa_act_forward(const void* x, void* y, const void* up12, const void* dn12, const void* log_alpha,
                       const void* log_beta, int B, int C, int T, int dtype, gsv_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * single-kernel test entry points
 * ------------------------------------------------------------------------------------- */
typedef struct {
  const void* x; const void* w; const float* bias; void* y; const void* res;
  int T_in, T_out, Cin, Cout, taps, stride, dil, pad;
  int pre_act; float pre_slope; int post_act; float scale; int accumulate; int out_f32;
  int ups_u, ups_pad;
  /* optional (0 = defaults): batched GEMM over Z slices with element strides, explicit leading dims */
  int Z; long long xz, wz, yz; int ldx, ldw, ldy;
  const float* gate;   /* optional per-output-channel gate: y = ((W x + b) * gate + res) * scale */
  int bz;              /* grouped convs (Z > 1): element stride of bias between slices (0 = one bias shared by all) */
  long long rz; int ldr; /* residual: element stride between slices (0 = yz) and leading dim (0 = ldy) */
  int res_dtype;       /* residual dtype: 0 = follows out_f32, 1 = fp32, 2 = the engine dtype (out_f32 with an fp16 residual) */
  int y_col0;          /* column offset of the written slice inside each y row (ldy must cover it) */
  int w_nt;            /* weights loaded non-temporal (GEMM paths) */
  int z_res;           /* batched launch (Z > 1) with a residual of its own slice stride rz: may take the LDS GEMM path */
  int gate_rows;       /* > 0: per-row gates, output row t is gated by gate + (t / gate_rows) * gate_ld (fp32 [rows / gate_rows][gate_ld]) */
  int gate_ld;         /*      instead of the one vector at gate; Z = 1, taps-1 GEMMs and the generic kernel (csrc/common.h ConvArgs) */
} gsv_conv_desc;
/* fused softmax attention of the DiT blocks alone (fp16, head dim 64): qkv [dev] f16 [T][3*heads*64] (q | k | v column
 * blocks), vt_scratch [dev] heads*64*ceil32(T) halfs, out [dev] f16 [T][heads*64] */
int gsv_op_flash_attn64(const void* qkv, int T, int heads, float scale, void* vt_scratch, void* out, gsv_stream_t stream);
/* the same attention over n_seg sequences packed back to back (the batched zh BERT pass): qkv [dev] f16 [sum T][3*heads*64],
 * seg_lens [host] n_seg lengths T_s >= 1, out [dev] f16 [sum T][heads*64]; query i of segment s attends to the keys of segment s
 * only.  Two launches for all segments, no host synchronisation and no allocation in the call (the segment table travels in one
 * small async copy on `stream` from a page-locked buffer the library owns).  vt_scratch [dev]: heads * 64 * 32 * sum ceil(T_s / 32)
 * halfs, 16-byte aligned, may arrive uninitialised (segment s owns V^T columns 32 * sum_{s' < s} ceil(T_s' / 32) onwards, its
 * padding columns are written as 0).  n_seg < 1, n_seg > 8192 or a T_s < 1 is GSV_ERR_ARG. */
int gsv_op_flash_attn64_seg(const void* qkv, int n_seg, const int32_t* seg_lens, int heads, float scale, void* vt_scratch, void* out,
                            gsv_stream_t stream);
/* test hook: gsv_op_flash_attn64 over `rows` utterances of T frames in one call (launch_flash_attn64_f16_rows, the DiT's batched
 * launch), with the rotary plane and a choice of kernel instantiation.  Strides are padded so that a stride mistake shows:
 * qkv [dev] f16 [rows][T + 8][3*heads*64] (the 8 rows behind every utterance are never read), out [dev] f16 [rows][T + 8][heads*64]
 * (the 8 rows are never written), vt_scratch [dev] rows * (heads*64*ceil32(T) + 64) halfs, may arrive uninitialised.  rope_cs
 * [dev] fp32 [T][rope_half][2] (cos, sin) or NULL: q and k are rotated IN PLACE on the first 2*rope_half channels of the un-split
 * projection (interleaved pairs (2p, 2p+1)) before the attention, every row with the same table.  qt: 0 = query tiles per
 * workgroup by the launcher's rule (GSV_FLASH_QT included), 1 / 2 / 4 = that instantiation.  GSV_ERR_ARG before any launch: a null
 * pointer, T / rows / heads < 1, qt outside {0, 1, 2, 4}, rope_half < 0 or 2*rope_half > heads*64, rope_half > 0 without a table. */
int gsv_op_flash_attn64_rows(const void* qkv, int T, int heads, int rows, float scale, const float* rope_cs, int rope_half, int qt,
                             void* vt_scratch, void* out, gsv_stream_t stream);
/* test hook: gsv_op_flash_attn64_seg with the same qt argument */
int gsv_op_flash_attn64_seg_qt(const void* qkv, int n_seg, const int32_t* seg_lens, int heads, float scale, int qt, void* vt_scratch,
                               void* out, gsv_stream_t stream);
/* test hook: one multi-head attention through the engines' own attention() (csrc/engine.hip) on a temporary context: it allocates
 * the workspaces, uploads kr, waits for the kernels and frees.  q [dev] [Tq][ldq], head h at columns qcol0 + h*kc ..; kv [dev]
 * [Tk][ldkv] with K at kcol0 + h*kc .. and V at vcol0 + h*kc ..; out [dev] [Tq][ldo]; dtype GSV_F16 / GSV_F32 applies to all
 * three.  rel_k / rel_v [dev] fp32 [9][kc] or both NULL: window-4 relative positions (key j of query i at offset j - i).  kr [host] int32 [2*Tq] or
 * NULL: query i sees keys [kr[2i], kr[2i+1]) only; an empty range gives a zero row on the materialised route.  route: 0 = what the
 * engine takes (fused for fp16, kc 96, both tables, q == kv, ldq == ldkv, unless GSV_MATERIALIZED_ENC_ATTN is set), 1 = the fused
 * flash_rel96 kernel, 2 = the materialised path (scores GEMM, row softmax, V transpose, PV GEMM, relative-value add).
 * GSV_ERR_ARG before any launch: a null q / kv / out, an unknown route or dtype, a shape < 1, head columns outside a leading
 * dimension, one relative table without the other, route 1 with GSV_F32, kc != 96, no tables or Tq != Tk, a key range outside
 * [0, Tk] or with hi < lo, and on the fused route a range that is empty or whose lo or hi is below the previous query's (the
 * kernel skips chunks by its first row's lo and last row's hi). */
int gsv_op_attention(const void* q, int ldq, int qcol0, const void* kv, int ldkv, int kcol0, int vcol0, int Tq, int Tk, int heads, int kc,
                     float scale, const float* rel_k, const float* rel_v, const int32_t* kr, int dtype, int route, void* out, int ldo,
                     gsv_stream_t stream);
/* test hook: the last attention launch on this thread (0 = none since the last reset): byte 0 = family (1 flash_attn64 rows,
 * 2 flash_attn64 segmented, 3 flash_rel96, 4 materialised), byte 1 = 16-query tiles per workgroup (0 for family 4). */
uint64_t gsv_debug_last_attn_route(int reset);
/* BERT's embedding stage: y[i] = LayerNorm(word[ids[i]] + pos[pos_ids[i]] + add) * gamma + beta as f16 rows [rows][C]; word [dev]
 * fp32 [n_word][C], pos [dev] fp32 [n_pos][C], add [dev] fp32 [C] or NULL, ids / pos_ids [dev] int32 [rows], gamma / beta [dev] fp32
 * [C]; sums and statistics in fp32.  C <= 1024.  A row whose id or position is outside its table is stored as NaN. */
int gsv_op_embed_ln(const float* word, int n_word, const float* pos, int n_pos, const float* add, const int32_t* ids,
                    const int32_t* pos_ids, const float* gamma, const float* beta, void* y, int rows, int C, float eps,
                    gsv_stream_t stream);
/* enc_p self-attention with window-4 relative positions alone (fp16, head dim 96, module/attentions.py:227-258):
 * qkv [dev] f16 [T][3*heads*96], rel_k / rel_v [dev] fp32 [9][96], vt_scratch heads*96*ceil32(T) halfs, out f16 [T][heads*96] */
int gsv_op_flash_rel96(const void* qkv, int T, int heads, float scale, const float* rel_k, const float* rel_v, void* vt_scratch,
                       void* out, gsv_stream_t stream);
/* the AR decode-step attention alone (reference t2s_model.py:176-221, one query per row over its cached keys; head dim 32):
 * q [dev] [B][H*32]; kc / vc [dev] [B][H][smax][32]; kv_len [dev] int32 [B]: row b attends to keys 0..kv_len[b] (the
 * current token's K/V already stored at position kv_len[b]); active [dev] int32 [B] (0 = row skipped, out untouched);
 * out [dev] [B][H*32].  dtype GSV_F16 / GSV_F32 applies to q, kc, vc, out. */
int gsv_op_decode_attn(const void* q, const void* kc, const void* vc, const int32_t* kv_len, const int32_t* active, int B, int H,
                       int smax, int dtype, void* out, gsv_stream_t stream);
/* the AR prefill's K/V fill and attention alone (csrc/t2s_prefill.hip; mask of t2s_model.py:655-683: text queries see the text
 * keys, audio queries all text keys plus the causal audio keys), through the routing code the engine itself launches with.  A
 * test hook: it uploads the row table, allocates the V^T scratch, waits for the kernels and frees.  qkv [dev] [M][3*d], the
 * rows of every utterance packed back to back ([x_0 .. x_{X_b-1} | y_0 .. y_{P_b-1}], M = sum S_b, S_b = x_len[b] + p_len[b]);
 * x_len / p_len [host] int32 [B]; d = 32 * H; kc / vc [dev] [B][H][smax][32], written at positions j < S_b only; out [dev]
 * [M][d].  dtype GSV_F16 / GSV_F32 applies to qkv, kc, vc, out.  route: 0 = what the engine takes for this dtype (the
 * GSV_SCALAR_PREFILL_ATTN / GSV_PREFILL_SPLIT_SCATTER switches included), 1 = fused K/V + V^T launch, then the MFMA flash kernel
 * (fp16 only), 2 = K/V scatter and V^T as two launches, then the flash kernel (fp16 only), 3 = K/V scatter + the scalar kernel.
 * GSV_ERR_ARG before any launch: a null pointer, d != 32 * H, x_len[b] < 1, p_len[b] < 0, S_b + 2 > smax, route 1 / 2 with
 * GSV_F32, an unknown route or dtype. */
int gsv_op_prefill_attn(const void* qkv, const int32_t* x_len, const int32_t* p_len, int B, int H, int d, int smax, int dtype,
                        int route, void* kc, void* vc, void* out, gsv_stream_t stream);
/* channels-last conv1d: x [T_in][Cin], w [Cout][taps*Cin] (tap-major, cin fastest), y [T_out][Cout] */
int gsv_op_conv1d(const gsv_conv_desc* d, int dtype, gsv_stream_t stream);
/* test hook: the same descriptor through the prefill's panel GEMM (csrc/gemm_panel.hip) instead of the dispatcher.  tile: 0 = the
 * launcher's choice by shape, 1 = 192 x 256, 2 = 192 x 192, 3 = 96 x 128 (rows x output channels), 4 = 96 x 128 with the
 * two-accumulator sum of gemm_t64 (even / odd k-steps of 16), which is what the dispatcher computes up to 2048 rows.  Eligible: GSV_F16, taps 1,
 * stride 1, pad 0, Z <= 1, Cin % 64 == 0, Cout % 8 == 0, y_col0 0, 16-byte aligned operands, a bias, no gate / accumulate /
 * pre-activation / transposed form, and one of: fp16 out (post_act none or ReLU) | fp32 out + fp16 residual (res_dtype 2, no
 * activation).  Anything else, or an unknown tile, is GSV_ERR_ARG before any HIP call; outputs are then untouched.  Bit-identical
 * to what gemm_lds (tiles 0..3) or gemm_t64 (tile 4) computes for the same rows. */
int gsv_op_gemm_panel(const gsv_conv_desc* d, int dtype, int tile, gsv_stream_t stream);
/* test hook: which kernel instantiation the last gsv_op_conv1d / gsv_op_conv_pair / engine conv launch on this thread ran
 * (0 = none since the last reset).  Byte fields, low to high: family, dtype (GSV_F32 / GSV_F16), five template parameters p0..p4,
 * flags (1 RES, 2 ACCU, 4 ALLW, 8 WNT, 16 SEG, 32 GROWS = the per-row-gate instantiation of families 1, 2, 4, 7).  Families and their parameters:
 *   1 gemm_sk_f16 | 2 gemm_t64_f16 p0 = SLAB / 16 | 3 conv_wide_f16 p0 = waves | 4 gemm_lds p0 = waves, p1 = xcd_order
 *   5 conv_lds p0..p4 = TM, TN, WM, WN, CC | 6 conv_narrow_f16 p0..p3 = CC, TM, TN, WN | 7 conv_gemm (generic) p0..p3 = TM, TN, WM, WN
 *   8 conv_pair_f16 p0 = C, p1 = taps; flag SEG = the masked pair of a segmented decode (gsv_op_conv_pair_seg).
 *   9 gemm_panel_f16 p0 = tile rows / 32, p1 = tile output channels / 32, p2 = 1: gemm_t64's two-accumulator sum (the prefill's own
 *     GEMM, launched in front of the dispatcher)
 * reset != 0 clears the record after reading it. */
uint64_t gsv_debug_last_conv_route(int reset);
/* the same record for the last family-8 launch (gsv_op_conv_pair / gsv_op_conv_pair_seg / a fused pair inside an engine decode)
 * since the last reset.  A decode's last launch is conv_post, so its pairs are read here. */
uint64_t gsv_debug_last_pair_route(int reset);
/* y = LN(x (+res)) over the last dim C; all buffers of `dtype`, gamma/beta fp32 */
int gsv_op_layernorm(const void* x, const void* res, const float* gamma, const float* beta, void* y, int rows,
                     int C, float eps, int dtype, gsv_stream_t stream);
/* the per-row low-rank delta of the adapted DiT passes (csrc/lora.hip), a test hook that waits for the kernel: x [dev]
 * [DB * Tn][K] and y [dev] [DB * Tn][N] of `dtype`; row b (its Tn frames) with s = slots[b] >= 0 ([host] DB ints, -1 = leave
 * the row alone) gets y += gate (.) ((x A_s^T) B_s^T).  blocks [host] n_slots device pointers: block s is A_s
 * [n_proj * rp[s]][K] followed by B_s [N][rp[s]] in `dtype`, rp[s] ([host]) the rank padded to a multiple of 16 (16 .. 128);
 * output column c contracts with columns [p * rp, (p + 1) * rp) of x A_s^T, p = c / (N / n_proj).  gate [dev] fp32 [N] or
 * NULL.  K a multiple of 32, N / n_proj a multiple of 16, n_proj 1 .. 3. */
int gsv_op_lora_delta(const void* x, void* y, int Tn, int DB, int K, int N, int n_proj, const int* slots, int n_slots,
                      const void* const* blocks, const int* rp, const float* gate, int dtype, gsv_stream_t stream);
/* reference-audio front-end helpers (host orchestration in gsv/module/mel_processing.py and
 * gsv/feature_extractor/cnhubert.py, the GEMMs are gsv_op_conv1d):
 *  gsv_op_frame: out[t][k] = x[reflect(t*hop + k - pad)], k < frame_len, zero up to ld; x [dev] fp32 [n]; out [T_out][ld] of dtype
 *    (torch.stft's reflect framing, reference module/mel_processing.py:55-71; pad = 0: the operand of a strided Conv1d(1, C, k))
 *  gsv_op_magnitude: re_im [dev] fp32 [T][2*bins] (re | im) -> sqrt(re^2 + im^2 + eps) (:73) as spec [dev] fp32 [bins][T]
 *    (frame_ld = 0), or frame-major [T][frame_ld] zero-filled beyond bins (the operand of the mel-filterbank GEMM, :138-140);
 *    eps < 0: the power spectrum re^2 + im^2 (Kaldi fbank use_power, eres2net/kaldi.py:612-614)
 *  gsv_op_channel_norm: channels-last [T][C]: per-channel mean / biased variance over T, affine, activation (ACT codes of
 *    gsv_conv_desc.post_act) -- torch.nn.GroupNorm(C, C) of the HuBERT feature extractor; scratch [dev] 128*C floats
 *  gsv_op_aff_mix: out = x (1 + t) + y (1 - t) over n fp32 elements (eres2net/fusion.py:22-27, t = tanh of the attention branch)
 *  gsv_op_time_mean: x [dev] fp32 [T][ld] -> out[ld] = mean over T (ERes2NetV2.forward3, eres2net/ERes2NetV2.py:258) */
int gsv_op_frame(const float* x, int n, int frame_len, int hop, int pad, int ld, int T_out, void* out, int dtype, gsv_stream_t stream);
int gsv_op_magnitude(const float* re_im, int T, int bins, float eps, int frame_ld, float* spec, gsv_stream_t stream);
/* one HiFi-GAN ResBlock pair of the generator's narrow stages in one kernel (fp16, C = 16 or 32, reference module/models.py:262-283):
 * y = (convs2(lrelu(convs1(lrelu(x)))) + x) * scale [+ y]; x, y [dev] f16 [T][C] (y must not alias x); w1 / w2 [dev] f16 [C][taps*C]
 * tap-major, convs1 dilated by `dil`, convs2 dilation 1; b1 / b2 [dev] fp32 [C].  Same rounding points as two gsv_op_conv1d launches. */
int gsv_op_conv_pair(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int T, int C, int taps,
                     int dil, float scale, int accumulate, gsv_stream_t stream);
/* the same pair inside a segmented decode (gsv_vits_decode_segments): row_seg [dev] int32 [T], the row's segment or -1 for a gap
 * row.  Gap rows of the intermediate are 0 to convs2 and gap rows of y are stored as 0 whatever bias, residual, scale or accumulate
 * give: bit-identical to convs1 -> zero the gap rows -> convs2 -> zero the gap rows.  x must hold 0 in its gap rows.
 * row_seg == NULL is GSV_ERR_ARG. */
int gsv_op_conv_pair_seg(const void* x, const void* w1, const float* b1, const void* w2, const float* b2, void* y, int T, int C, int taps,
                         int dil, float scale, int accumulate, const int32_t* row_seg, gsv_stream_t stream);
/* BigVGAN's anti-aliased snake / snakebeta on channels-last activations, the kernel the vocoder engine runs: x, y [dev] [T][C] of
 * dtype, alpha / beta [dev] fp32 [C] (logscale != 0: stored as logarithms).  row_seg == NULL: replicate padding at rows 0 and
 * T - 1.  Otherwise the form of a segmented pass (gsv_vocoder_forward_segments): row_seg [dev] int32 [T], the row's segment or -1
 * for a gap row; seg_start / seg_len [dev] int32 [n_seg], segment s covers rows [seg_start[s], seg_start[s] + seg_len[s]).  Both
 * replicate paddings stop at the row's own segment, gap rows of y are stored as 0 and gap rows of x are never used. */
int gsv_op_aa_act_cl(const void* x, void* y, int T, int C, const float* alpha, const float* beta, int logscale,
                     const int32_t* row_seg, const int32_t* seg_start, const int32_t* seg_len, int n_seg, int dtype,
                     gsv_stream_t stream);
int gsv_op_aff_mix(const float* x, const float* y, const float* t, long long n, float* out, gsv_stream_t stream);
int gsv_op_time_mean(const float* x, int T, int ld, float* out, gsv_stream_t stream);
int gsv_op_channel_norm(const void* x, int T, int C, const float* gamma, const float* beta, float eps, int act, float* scratch,
                        void* y, int dtype, gsv_stream_t stream);
/* gsv_op_channel_norm over n_seg row ranges of one channels-last array (the packed HuBERT pass, gsv/feature_extractor/cnhubert.py
 * HubertModel.batch: GroupNorm(C, C) over each audio's own rows): x, y [dev] [T][C] of dtype (f16 / f32), 16-byte aligned, C a
 * multiple of 8 (f16) / 4 (f32); seg_start / seg_len [host] n_seg ranges [start, start + len), disjoint and ascending, len >= 1,
 * inside [0, T).  Rows of segment s: y = act((x - mean_{s,c}) * rstd_{s,c} * gamma[c] + beta[c]), mean and biased variance over the
 * segment's own rows (fp32 partial sums of x minus the segment's first row, per 256 rows counted from that row, summed in order in
 * double precision);
 * every other row of y is stored as 0.  A segment's output bits depend on its own rows alone, not on its position or on the other
 * segments of the call.  Three launches, no host synchronisation and no allocation in the call (the table travels like
 * gsv_op_flash_attn64_seg's).  scratch [dev] fp32: 2 * C * (sum_s ceil(len_s / 256) + n_seg) floats, may arrive uninitialised.
 * n_seg < 1, n_seg > 8192, a len < 1, overlapping or descending segments, or one that ends past T: GSV_ERR_ARG. */
int gsv_op_channel_norm_seg(const void* x, int T, int C, int n_seg, const int32_t* seg_start, const int32_t* seg_len,
                            const float* gamma, const float* beta, float eps, int act, float* scratch, void* y, int dtype,
                            gsv_stream_t stream);
/* y[r] = x[idx[r]] for r < rows_out: x [dev] [rows_in][C], y [dev] [rows_out][C] of dtype (f16 / f32), rows a multiple of 16 bytes
 * and both arrays 16-byte aligned, idx [dev] int32 [rows_out].  idx[r] < 0 stores a zero row (the gap rows the packed HuBERT pass
 * puts between audios in front of the positional conv); idx[r] >= rows_in stores a NaN row, as gsv_op_embed_ln does for an id
 * outside its table.  x and y must not overlap. */
int gsv_op_gather_rows(const void* x, int rows_in, const int32_t* idx, int rows_out, int C, void* y, int dtype, gsv_stream_t stream);
/* the two segmented kernels of the packed speaker-embedding pass (gsv/eres2net/ERes2NetV2.py forward3_segments, DESIGN.md
 * section 4l), where the audios lie back to back on the time axis with gap rows between them.
 * gsv_op_zero_rows: stores 0 to rows rows[0 .. n_rows) of n_maps (1 .. 8) fp32 maps [T][ld] of one shape, in one launch: the gap
 *   rows in front of a conv that reads across time.  maps->p[0 .. n_maps) [dev], 16-byte aligned, ld a multiple of 4 floats; the
 *   row list comes twice, rows [dev] int32 [n_rows] for the kernel and rows_host [host], the same n_rows values, for the check
 *   (so the call neither waits for the device nor copies): a row outside [0, T), ld % 4 != 0 or n_maps outside 1 .. 8 is
 *   GSV_ERR_ARG.  The kernel skips a device row outside [0, T).  Every other element of the maps is left as it is.
 * gsv_op_time_mean_seg: x [dev] fp32 [T][ld] -> out [dev] fp32 [n_seg][ld], out[s] = mean over the rows [seg_start[s],
 *   seg_start[s] + seg_len[s]) in gsv_op_time_mean's order counted from the segment's first row (16 strided slices, the 16
 *   partials in order, divided by the length): a segment's bits depend on its own rows alone, and one segment [0, T) gives
 *   gsv_op_time_mean's bits.  seg_start / seg_len [host], checked as gsv_op_channel_norm_seg checks them (1 .. 8192 segments,
 *   len >= 1, disjoint and ascending, inside [0, T)); ld a multiple of 4, x and out 16-byte aligned; the table travels like
 *   gsv_op_flash_attn64_seg's, so the call neither waits nor allocates. */
typedef struct gsv_zero_maps { float* p[8]; } gsv_zero_maps;
int gsv_op_zero_rows(const gsv_zero_maps* maps, int n_maps, int T, int ld, const int32_t* rows, const int32_t* rows_host, int n_rows,
                     gsv_stream_t stream);
int gsv_op_time_mean_seg(const float* x, int T, int ld, int n_seg, const int32_t* seg_start, const int32_t* seg_len, float* out,
                         gsv_stream_t stream);
/* the device front-end of a voice enrolment (TTS.make_voices(device_frontend=True)): the reference audios
 * lie back to back in one fp32 stream.
 * gsv_op_resample_poly_seg: rational polyphase FIR resampling of n_seg segments of x [dev] fp32 [n_x] into y [dev] fp32 [n_y], the
 *   arithmetic of scipy.signal.resample_poly(x, up, down, padtype="constant") with the filter handed in: h [dev] fp32 [h_len],
 *   h_len = 2 * half + 1 (odd); the op designs nothing.  Segment s = x[in_start[s] .. + in_len[s]) has m_s = ceil(in_len[s] * up /
 *   down) outputs at y[out_start[s] .. + m_s):  y_s[i] = sum_j h[i * down + half - j * up] * x_s[j] over the j in [0, in_len[s])
 *   whose filter index lies in [0, h_len) -- samples of other segments never enter, the edges see zeros.  One fp32 accumulator per
 *   output over its taps in ascending j (fused multiply-add): a segment's output bits depend on its own samples alone, not on its
 *   position, its neighbours or the call's other segments.  Elements of y outside every output range are left as they are.
 *   peak [dev] fp32 [n_seg] or NULL: peak[s] = max_i |y_s[i]| (the call zeroes it first).  in_start / in_len / out_start [host]
 *   travel like gsv_op_flash_attn64_seg's table: the call neither waits nor allocates.  GSV_ERR_ARG before any launch: n_seg
 *   outside 1 .. 8192, a length < 1, up or down < 1, an even h_len, input or output ranges that overlap, descend or leave
 *   [0, n_x) / [0, n_y), h_len > 65535, or an input window per 1024 outputs ((1023 * down + h_len - 1) / up + 2 samples) above
 *   16384.  The filter is staged in LDS when window + h_len <= 16384 floats (every pair among 16 / 22.05 / 24 / 32 / 44.1 / 48 kHz
 *   with resample_poly's default filter, h_len = 20 * max(up, down) + 1 <= 12801), else it is read through L2.
 * gsv_op_frame_seg: gsv_op_frame per segment: rows [row_start[s], row_start[s] + row_len[s]) of out [dev] [rows][ld] of dtype hold
 *   x[x_start[s] + reflect_s(t * hop + k - pad)], t counted from the segment's first row, reflected at the segment's own ends,
 *   zero up to ld -- the bits of gsv_op_frame on that audio alone.  Rows outside every range are left as they are.  x_start /
 *   x_len / row_start / row_len [host], 1 .. 8192 segments, sample and row ranges disjoint and ascending inside [0, n_x) and
 *   [0, rows), pad < x_len[s], and the frames of a segment inside its padded signal; else GSV_ERR_ARG.  One launch. */
int gsv_op_resample_poly_seg(const float* x, int n_x, const float* h, int h_len, int up, int down, int n_seg, const int32_t* in_start,
                             const int32_t* in_len, const int32_t* out_start, float* y, int n_y, float* peak, gsv_stream_t stream);
int gsv_op_frame_seg(const float* x, int n_x, int frame_len, int hop, int pad, int ld, int n_seg, const int32_t* x_start,
                     const int32_t* x_len, const int32_t* row_start, const int32_t* row_len, int rows, void* out, int dtype,
                     gsv_stream_t stream);
/* sampling kernel alone: logits [dev] fp32 [B][vocab], prev [dev] int32 [B][prev_len], noise [dev]
 * fp32 [B][vocab] or NULL; outputs [dev] int32 [B]: sampled token, argmax of penalised logits */
int gsv_op_sample(const float* logits, int B, int vocab, int vocab_eff, const int32_t* prev, int prev_len,
                  const gsv_sampling_params* sp, const float* noise, int step, int32_t* sampled,
                  int32_t* argmax_tok, gsv_stream_t stream);
/* the same with one gsv_row_sampling_t per row, rows [host] [B] (checked like gsv_t2s_set_row_sampling), and the counter-RNG
 * seed as an argument; waits for the kernel (a test hook) */
int gsv_op_sample_rows(const float* logits, int B, int vocab, int vocab_eff, const int32_t* prev, int prev_len,
                       const gsv_row_sampling_t* rows, uint64_t seed, const float* noise, int step, int32_t* sampled,
                       int32_t* argmax_tok, gsv_stream_t stream);
/* the log-probability of gsv_t2s_set_logprobs alone, one wave per row: logits [dev] fp32 [B][vocab], tokens [dev] int32 [B];
 * out [dev] fp32 [B] = log softmax(logits[b][:vocab_eff])[tokens[b]], -inf for a token outside [0, vocab_eff) */
int gsv_op_token_logprob(const float* logits, int B, int vocab, int vocab_eff, const int32_t* tokens, float* out,
                         gsv_stream_t stream);

/* Monotonic alignment of a text-to-frame attention (csrc/align.hip).  A call carries n spans; span i is the rectangle of frame
 * rows [f0, f0 + nf) of q [.][ldq] and phoneme rows [l0, l0 + nl) of k [.][ldk], both [dev] in `dtype`, `heads` heads of
 * `head_dim` columns each from column 0.  spans [dev] [n]; spans are independent: a span's outputs do not depend on what else
 * the call holds.
 *   gsv_op_align_logp: lp[t][j] = logf(max(1e-30, mean_h softmax_j(scale * <q_h[t], k_h[j]>))), fp32, the softmax over the
 *     span's own nl phonemes, written [nf][nl] at the span's place in the workspace.
 *   gsv_op_align_path: VITS' maximum_path over lp, V in fp64: V[0][0] = lp[0][0], V[t][j] = lp[t][j] + max(V[t-1][j],
 *     V[t-1][j-1]), j <= t; the backtrack from (nf - 1, nl - 1) steps to j - 1 iff j > 0 && (j == t || V[t-1][j] < V[t-1][j-1])
 *     (a tie stays).  ends [dev] int32: ends[out0 + j] = the exclusive end frame of phoneme j inside the span (its start is the
 *     previous end, every phoneme gets >= 1 frame); score [dev] fp32 [n]: (float)(V[nf-1][nl-1] / nf).  A span with nf < nl or
 *     nl > 1024 is not searched: ends[out0 + j] = ((j + 1) * nf) / nl and score = -inf; nf <= 0 or nl <= 0 writes no ends and
 *     score = -inf.
 *   gsv_op_align: both launches.
 * Workspace [dev], 16-byte aligned: gsv_op_align_workspace(n, spans [host], offsets) returns its size in bytes (negative: bad
 * table) and, when offsets is not NULL, the byte offset of each span's lp (offsets [host] [n]); a searched span takes
 * nf * nl floats rounded up to 16 bytes, plus its decision bits when they exceed 32 KB, an unsearched one nothing.  A span whose
 * region would pass workspace_bytes takes the fallback.  Nothing is allocated and nothing waits for the device. */
typedef struct gsv_align_span {
  int32_t f0, nf; /* frame rows of q */
  int32_t l0, nl; /* phoneme rows of k */
  int32_t out0;   /* first element of `ends` the span writes */
  int32_t reserved;
} gsv_align_span_t;
long long gsv_op_align_workspace(int n_spans, const gsv_align_span_t* spans, int64_t* offsets);
int gsv_op_align_logp(const void* q, int ldq, const void* k, int ldk, int dtype, int heads, int head_dim, float scale,
                      const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, gsv_stream_t stream);
int gsv_op_align_path(const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, int32_t* ends,
                      float* score, gsv_stream_t stream);
int gsv_op_align(const void* q, int ldq, const void* k, int ldk, int dtype, int heads, int head_dim, float scale,
                 const gsv_align_span_t* spans, int n_spans, void* workspace, long long workspace_bytes, int32_t* ends, float* score,
                 gsv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GSV_H_ */
