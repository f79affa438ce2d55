/*
 * voitta_engine.h — C-ABI of libvoitta_engine.so, the MI355X (gfx950) in-process
 * indexing-and-retrieval engine that replaces, for voitta-rag's hot path only,
 *   - sentence-transformers' encode          (reference: src/voitta/services/embedding.py:40-86)
 *   - fastembed's Qdrant/bm25 sparse vectors  (reference: src/voitta/services/sparse_embedding.py:18-50,
 *                                              scripts/build_sparse_vectors.py:124,170)
 *   - the Qdrant client calls on the path     (reference: src/voitta/services/vector_store.py:233-317
 *                                              upsert, :560-697 search / hybrid fusion, :462-530 filters,
 *                                              :319-434 deletes)
 *
 * The reference has no FFI of its own (it is 100 % Python); these entry points are what a ctypes
 * binding inside the three service classes would call. Plain pointers and sizes only — no torch,
 * numpy or C++ types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; vr_last_error() returns a thread-local
 *     message (the Python side raises RuntimeError with it — reference callers catch broadly:
 *     src/voitta/services/indexing.py:531-533,561-563).
 *   - `mem` arguments say where the caller's buffers live: VR_MEM_HOST (pageable host memory,
 *     e.g. numpy) or VR_MEM_DEVICE (HBM of the engine's device, e.g. a torch-ROCm tensor).
 *     Output buffers follow the same `mem` unless stated otherwise.
 *   - row ids are dense int64 indices into the engine's HBM-resident tables, assigned in upsert
 *     order; the UUID<->row map and the text payload stay in the Python host.
 *   - thread-safety: one engine may be called from any number of threads. Searches run CONCURRENTLY, each on
 *     its own HIP stream with its own staging area ("lanes", VR_SEARCH_LANES of them, default 4; further
 *     searches wait for a free one), and hold a shared lock on the index for their duration. Mutations
 *     (vr_upsert, vr_index_batch(_spans), vr_delete_rows, vr_compact, vr_load) and vr_encode(_spans) are serialised among
 *     themselves and take the exclusive lock only to PUBLISH: the append of a batch, the tombstones of a
 *     delete, the pointer swap of a compaction (which builds its result beside the live index). A search
 *     therefore sees the state before or after a mutation, never a mixture, and waits for no encode and
 *     no compaction (the reference's callers: watcher.py:149-171,
 *     indexing.py:281-288, api/routes/folders.py:137-143 beside MCP search threads).
 *   - there is NO CPU fallback: creating an engine without a usable gfx950 device fails.
 */
#ifndef VOITTA_ENGINE_H
#define VOITTA_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 1

#define VR_MEM_HOST   0
#define VR_MEM_DEVICE 1

/* "field absent" marker for the source_created_at / source_modified_at columns
 * (reference stores the keys only when non-None: vector_store.py:279-282; a point lacking the
 * key fails a range `must`). */
#define VR_TS_ABSENT INT64_MIN

/* fusion modes for vr_search_hybrid */
#define VR_FUSION_MINMAX 0 /* reference behaviour: vector_store.py:659-689 */
#define VR_FUSION_RRF    1 /* north_star extra mode; no reference oracle */

typedef struct vr_engine vr_engine;

typedef struct vr_config {
  int32_t struct_size;   /* = sizeof(vr_config) */
  int32_t device;        /* HIP device ordinal */
  int32_t dim;           /* dense dimension D (multiple of 16, <= 1024): settings.embedding_dimension, embedding.py:20 */
  int32_t flags;         /* VR_ENGINE_* bits */
  int64_t initial_rows;  /* capacity hint; tables grow by doubling */
} vr_config;

/* vr_config.flags.
 * By default a single-query dense search over a store with dim % 32 == 0 runs in two stages:
 * a reduced-precision shadow copy of the corpus is scanned on the matrix cores — int8 with one
 * scale per row when dim % 64 == 0 (1/4 of the bytes, +25 % memory), f16 otherwise or when the
 * environment has VR_PREFILTER=f16 (1/2 of the bytes, +50 % memory) — a rigorous per-row error
 * bound (the norm of the row's quantisation residual, Cauchy-Schwarz) turns the approximate
 * scores into lower/upper bounds, and every row whose upper bound reaches the k-th best lower
 * bound is re-scored with the exact f32 chain. Results are bit-identical to the one-stage exact
 * scan (tests run both); the flag below turns the shadow copy and the first stage off. */
#define VR_ENGINE_NO_PREFILTER 1

/* Search-time predicate; restates _build_filter, vector_store.py:462-530. All ids are the
 * host's dictionary ids of folder_path / index_folder strings (exact string equality in the
 * reference => integer equality here). Arrays are host pointers and are tiny. */
typedef struct vr_filter {
  int32_t struct_size;
  int32_t n_must_folder_sets;       /* number of `must` any-of sets on folder_path (0..2):
                                       folder_filter (:476-482) and include_folders (:484-490) */
  const int32_t* must_folder_ids;   /* concatenated sets */
  const int32_t* must_folder_off;   /* n_must_folder_sets+1 offsets into must_folder_ids */
  const int32_t* not_folder_ids;    /* exclude_folders on folder_path (:492-499) */
  int32_t n_not_folder;
  int32_t n_not_index_folder;
  const int32_t* not_index_folder_ids; /* exclude_index_folders on index_folder (:501-508) */
  int32_t has_date_start;           /* gte (:514-515) */
  int32_t has_date_end;             /* lte (:516-517) */
  int64_t date_start;
  int64_t date_end;
  int32_t date_field;               /* 0 = source_modified_at (default), 1 = source_created_at (:511-512) */
  int32_t reserved0;
} vr_filter;

/* ---- lifecycle ---------------------------------------------------------------------------- */
int  vr_abi_version(void);
const char* vr_last_error(void);
int  vr_engine_create(const vr_config* cfg, vr_engine** out);
void vr_engine_destroy(vr_engine* e);
/* block until every kernel queued by previous calls has finished (for timing) */
int  vr_sync(vr_engine* e);
/* the engine's hipStream_t, as an opaque pointer (bench.py records HIP events on it) */
void* vr_stream(vr_engine* e);
/* queue all further work on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)
 * so that VR_MEM_DEVICE buffers produced on that stream need no extra synchronisation.
 * NULL rebinds the engine's own stream, which is a blocking stream (ordered against the legacy
 * null stream). Device buffers handed to the engine must be ready on the bound stream. */
int  vr_set_stream(vr_engine* e, void* stream);

/* ---- dense encode: replaces SentenceTransformer(...).encode (embedding.py:40,53,68-73,85) ----- */
#define VR_POOL_MEAN 0
#define VR_POOL_CLS  1
/* the final hidden row of the sequence's LAST token (decoder-style embedders: under a causal mask the only row that has
 * seen the whole sequence). Any encoder accepts it; a reranker does not; span calls ignore it as they ignore CLS. */
#define VR_POOL_LAST 2

/* BERT-family encoder description; values come from the checkpoint's config.json /
 * sentence-transformers modules.json (SURVEY.md §8 model table). */
typedef struct vr_bert_desc {
  int32_t struct_size;
  int32_t layers;
  int32_t hidden;        /* H: multiple of 128, <= 1024 */
  int32_t heads;         /* H / heads must be 32 or 64 (vr_bert_desc_v3.head_dim sets the head size on its own) */
  int32_t intermediate;  /* multiple of 128 */
  int32_t vocab;
  int32_t max_pos;       /* max_position_embeddings; also the longest accepted sequence. VR_POS_ROTARY: the length of
                          * the cos/sin table the engine builds, which is again the longest accepted sequence.
                          * VR_POS_NONE: there is no table, the longest accepted sequence alone. 1 .. 8192 */
  int32_t type_vocab;
  int32_t pooling;       /* VR_POOL_MEAN | VR_POOL_CLS | VR_POOL_LAST (sentence-transformers Pooling module) */
  int32_t normalize;     /* 1 = L2-normalise (sentence-transformers Normalize module) */
  float   eps;           /* layer_norm_eps */
  int32_t precision;     /* VR_PRECISION_F32 | VR_PRECISION_F16X3 | VR_PRECISION_F16 */
  /* Added after the first release: zero in every field below is the behaviour of a description that ends at
   * `precision` (struct_size may still be that shorter size; the missing fields are then read as zero). */
  int32_t position;      /* VR_POS_LEARNED | VR_POS_ROTARY | VR_POS_NONE */
  float   rope_theta;    /* VR_POS_ROTARY: base of the rotary frequencies, inv_freq_i = theta^(-2i/d_h); > 0 */
  int32_t ffn;           /* VR_FFN_GELU | VR_FFN_SWIGLU | VR_FFN_GEGLU | VR_FFN_RELU */
  /* Added with the pre-norm family (ModernBERT): again zero in every field is the behaviour of a description that
   * ends at `ffn`, and struct_size may be that shorter size. */
  int32_t norm;          /* VR_NORM_POST | VR_NORM_PRE | VR_NORM_PRE_RMS | VR_NORM_PRE_RMS_ROTARY */
  int32_t window;        /* sliding-window attention: the half-width w, 0 .. 4096. 0: every layer attends globally.
                          * Otherwise query i of a windowed layer sees key j of its own sequence iff |i - j| <= w */
  int32_t global_every;  /* window > 0: layer l attends globally iff l % global_every == 0 (>= 1), the rest are windowed */
  float   rope_theta_local; /* the rotary base of the windowed layers; 0 = rope_theta */
} vr_bert_desc;

/* vr_bert_desc and what was added behind it with the decoder-style embedders (Qwen2). vr_bert_desc itself keeps its
 * size and its fields; this is the same description one field longer, and vr_encoder_load / vr_reranker_load take either:
 * pass &v2.base with base.struct_size = sizeof(vr_bert_desc_v2). A vr_bert_desc of any accepted size reads `causal` as 0. */
typedef struct vr_bert_desc_v2 {
  vr_bert_desc base;
  int32_t causal;        /* 0: every query sees every key of its own sequence. 1: query i sees key j of its own sequence
                          * iff j <= i. VR_NORM_PRE_RMS_ROTARY only: every other norm refuses 1, and so does a reranker */
} vr_bert_desc_v2;

/* ... and what was added behind that with Qwen3: a head size that is not hidden / heads, and a per-head RMSNorm on the
 * query and the key. Passed as &v3.v2.base with base.struct_size = sizeof(vr_bert_desc_v3); every shorter accepted size
 * reads both fields as 0. VR_NORM_PRE_RMS_ROTARY only: every other norm refuses a non-zero value, and so does a reranker. */
typedef struct vr_bert_desc_v3 {
  vr_bert_desc_v2 v2;
  int32_t head_dim;      /* 0: the head size is hidden / heads. 32, 64 or 128: the head size, whatever hidden is; the
                          * attention width A = heads * head_dim must then be a multiple of 128 and at most 2048. The
                          * query / key / value weights are [A, H], their biases [A], attention.output.dense is [H, A],
                          * and the engine's rows are [Q | K | V] of 3 A */
  int32_t qk_norm;       /* 0 or 1. 1: every head of the query and of the key is RMS-normalised over its head_dim values
                          * (eps as every other norm) and scaled by q_norm.weight / k_norm.weight before the rotation; a
                          * layer then has 20 slots, 18: q_norm.weight, 19: k_norm.weight, [head_dim] f32 each */
} vr_bert_desc_v3;

/* position: LEARNED adds a row of the position table to every token's embedding; ROTARY has no table — the query and
 * key of every head are rotated by the token's position inside its own sequence (rotate-half pairing: feature j with
 * j + d_h/2, as in HF apply_rotary_pos_emb; the full head is rotated). NONE has no table and no rotation: the
 * embeddings are word + token type, and the model sees order through vr_encoder_set_attention_slopes alone (ALiBi:
 * jina-embeddings-v2) or vr_encoder_set_attention_bias (T5). NONE needs VR_NORM_POST or VR_NORM_PRE_RMS, and no window. */
#define VR_POS_LEARNED 0
#define VR_POS_ROTARY  1
#define VR_POS_NONE    2
/* ffn: GELU is down(gelu(up(x))); the gated forms are down(act(gate(x)) * up(x)) with act = SiLU (SWIGLU) or the
 * exact-erf GELU (GEGLU). RELU is down(max(up(x), 0)), T5's DenseReluDense: 16 slots per layer like GELU, and
 * VR_NORM_PRE_RMS only. */
#define VR_FFN_GELU   0
#define VR_FFN_SWIGLU 1
#define VR_FFN_GEGLU  2
#define VR_FFN_RELU   3
/* norm: POST is BERT's x = LN(x + f(x)). PRE is x = x + attn(LN(x)), x = x + mlp(LN(x)) with one final LayerNorm; the
 * embedding LayerNorm stays in the stream and layer 0 has no attention norm. PRE needs VR_POS_ROTARY and a gated ffn;
 * a window needs VR_NORM_PRE (and so rotary positions). A reranker takes them together (a ModernBERT cross-encoder, see
 * vr_reranker_load) or not at all.
 * PRE_RMS is the T5 encoder: h = word[id] with NO embedding norm in the stream; per layer h += W_o attn(N_a(h)), then
 * h += W_down relu(W_up N_m(h)); out = N_f(h). Every N is RMSNorm, x * rsqrt(mean(x^2) + eps) * weight (T5LayerNorm: no
 * mean subtraction, no shift; the slot's bias is ignored and may be NULL). PRE_RMS needs VR_POS_NONE, VR_FFN_RELU,
 * window 0 and type_vocab 1 (anything else is refused with the field named); a reranker never takes it.
 * T5's logits are q.k + bias WITHOUT the 1/sqrt(d_h): the engine keeps its scale, and the loader multiplies the query
 * weight by sqrt(d_h) instead (exactly x8 at head size 64, one f32 rounding per weight at 32).
 * PRE_RMS_ROTARY is the Llama / Qwen2 block: h = word[id]; per layer h += W_o attn(rope(N_a(h))), then
 * h += W_down(act(gate(N_m(h))) * up(N_m(h))); out = N_f(h), every N an RMSNorm as under PRE_RMS. It needs
 * VR_POS_ROTARY, a gated ffn, window 0 and type_vocab 1 (anything else is refused with the field named), takes
 * vr_bert_desc_v2.causal 0 or 1, refuses vr_encoder_set_attention_bias and _slopes, and a reranker never takes it. PRE_RMS itself
 * stays the T5 form alone. PRE_RMS_ROTARY is also the one norm that takes vr_bert_desc_v3 (Qwen3): head sizes 32, 64
 * and 128 set by head_dim, rope(N_q(q)) and rope(N_k(k)) per head with qk_norm. */
#define VR_NORM_POST 0
#define VR_NORM_PRE  1
#define VR_NORM_PRE_RMS 2
#define VR_NORM_PRE_RMS_ROTARY 3

/* arithmetic of the encoder's matrix products:
 *   F32    every product on the f32-input MFMA (exact f32 fma chains) — 157 TFLOP/s peak
 *   F16X3  operands carried as (hi, lo) f16 pairs (22 significant bits), three f16-MFMA passes per
 *          product into an f32 accumulator — f32-class accuracy (measured |1-cos| < 1e-6 against
 *          the f32 path) at 16/3 of the f32-MFMA rate. Activations beyond f16's range (65504) are
 *          clamped. Attention, LayerNorm, GELU, pooling stay f32 in both modes.
 *   F16    operands rounded to f16 (weights pre-scaled by a power of two per tensor), one f16-MFMA pass,
 *          f32 accumulate; everything outside the matrix products stays f32. Measured |1-cos| vs the
 *          f64 oracle: see tests/test_encoder_gpu.py (north_star tolerance: 1e-4). */
#define VR_PRECISION_F32   0
#define VR_PRECISION_F16X3 1
#define VR_PRECISION_F16   2

/* tensors: 5 + 16*layers f32 arrays in `mem`, HF BertModel state-dict order and [out,in] layout:
 *   word_embeddings, position_embeddings, token_type_embeddings, embeddings.LayerNorm.{weight,bias},
 *   then per layer: query.{weight,bias}, key.{weight,bias}, value.{weight,bias},
 *   attention.output.dense.{weight,bias}, attention.output.LayerNorm.{weight,bias},
 *   intermediate.dense.{weight,bias}, output.dense.{weight,bias}, output.LayerNorm.{weight,bias}.
 * A gated ffn (VR_FFN_SWIGLU / VR_FFN_GEGLU) has 18 slots per layer (5 + 18*layers tensors): the 16 above, where
 * intermediate.dense.{weight,bias} is the UP projection [I,H], followed by the GATE projection's {weight [I,H], bias}.
 * VR_NORM_PRE: the LayerNorm slots keep their places in the dataflow — each holds the norm that FOLLOWS the residual
 * add it sits behind, and the residual stream bypasses it: embeddings.LayerNorm = the embedding norm (in the stream);
 * layer l's attention.output.LayerNorm = the norm in front of layer l's FFN (ModernBERT: layers.l.mlp_norm); layer l's
 * output.LayerNorm = the norm in front of layer l + 1's attention (layers.l+1.attn_norm), and for the last layer the
 * final norm (final_norm). Layer 0's attention reads the embedding norm's output as it is.
 * VR_NORM_PRE_RMS: the slots as under VR_NORM_PRE with one difference: embeddings.LayerNorm holds block 0's attention
 * norm (T5: block.0.layer.0.layer_norm) and the stream bypasses it too. Layer l's attention.output.LayerNorm =
 * block.l.layer.1.layer_norm, layer l's output.LayerNorm = block.l+1.layer.0.layer_norm, the last = final_layer_norm.
 * VR_NORM_PRE_RMS_ROTARY: the same slots, 18 per layer (the ffn is gated): embeddings.LayerNorm = layers.0.input_layernorm,
 * layer l's attention.output.LayerNorm = layers.l.post_attention_layernorm, layer l's output.LayerNorm =
 * layers.l+1.input_layernorm, the last = norm. Grouped-query checkpoints are brought to `heads` full K and V heads by
 * the loader (HF repeat_kv): the engine sees [Q | K | V] rows of 3 H (3 A with vr_bert_desc_v3.head_dim, and with
 * vr_bert_desc_v3.qk_norm two slots more per layer: q_norm.weight, k_norm.weight).
 * NULL slots: any bias (read as zeros), and position_embeddings when position is VR_POS_ROTARY or VR_POS_NONE (ignored
 * then); under VR_NORM_PRE_RMS and VR_NORM_PRE_RMS_ROTARY also every LayerNorm bias (ignored) and token_type_embeddings (read as zeros).
 * Every other slot must be non-NULL.
 * The engine copies (and re-packs) them; the caller's tensors may be freed afterwards.
 * Replaces EmbeddingService.model's lazy SentenceTransformer(...) load (embedding.py:23-42). */
int vr_encoder_load(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors,
                    int32_t n_tensors, int mem);

/* Additive attention bias of the loaded ENCODER, by relative offset: every layer's logit of query i against key j of
 * head h becomes q.k/sqrt(d_h) + table[h][clamp(j - i, -radius, radius) + radius]. table: heads x (2*radius + 1) f32
 * in `mem`, copied. 1 <= radius <= 512; heads must equal the loaded description's. Needs VR_POS_LEARNED and
 * VR_NORM_POST, or VR_POS_NONE and VR_NORM_PRE_RMS (refused otherwise, and while vr_encoder_set_attention_slopes' slopes are set; the encoder stays as it
 * was). NULL table removes the bias. vr_encoder_load resets it. The reranker never has one.
 * (MPNet: one T5-style bucketed table shared by all layers; its buckets depend on j - i alone and are constant from
 * |j - i| = 128 on, so radius 128 reproduces the model at any length. T5: block 0's relative_attention_bias, the same
 * buckets, constant from relative_attention_max_distance on.) */
int vr_encoder_set_attention_bias(vr_engine* e, const float* table, int32_t heads, int32_t radius, int mem);

/* Linear attention bias of the loaded ENCODER (ALiBi): every layer's logit of query i against key j of head h becomes
 * q.k/sqrt(d_h) - slopes[h] * |j - i|, at any distance (nothing saturates, no key is skipped). slopes: `heads` f32 in
 * `mem`, copied; each finite, 0 <= slope <= 1e30 (beyond that the bias of a far key would leave f32's range); heads
 * must equal the loaded description's. Needs VR_NORM_POST and VR_POS_LEARNED or VR_POS_NONE. Slopes and a table
 * (vr_encoder_set_attention_bias) never coexist: setting one while the other is set is refused. A refused call leaves
 * the encoder as it was. NULL slopes removes them. vr_encoder_load resets them. The reranker never has any. */
int vr_encoder_set_attention_slopes(vr_engine* e, const float* slopes, int32_t heads, int mem);

/* The post-pooling head of the loaded ENCODER: what a sentence-transformers pipeline runs behind Pooling (Dense and
 * LayerNorm modules, Normalize) and SentenceTransformer(truncate_dim=...). With a head a row is computed as
 *   1. the pooled row, un-normalised (vr_encode_spans: the span mean);
 *   2. the stages in order, all f32 whatever desc.precision is;
 *   3. if desc.normalize: x / max(|x|, 1e-12) over the WHOLE width of the last stage (or of the pooled row);
 *   4. the leading truncate_dim columns (0: all of them), not normalised again.
 * The OUTPUT WIDTH of the encoder is then truncate_dim, or else the last stage's out_dim, or else desc.hidden: vr_encode
 * and vr_encode_spans write rows of that width, and vr_index_batch(_spans) and vr_query_text(_batch), with their
 * Unigram and BPE variants, compare that width with the store dimension.
 * With no stages (pure truncation) a row is bit for bit the leading truncate_dim columns of the headless row.
 * Limits: 0 <= n_stages <= 4; every in_dim / out_dim a multiple of 16 in 16..1024; stages[0].in_dim == desc.hidden;
 * each stage's in_dim equals its predecessor's out_dim; a LayerNorm stage has in_dim == out_dim and eps > 0;
 * truncate_dim is 0 or a multiple of 16 not above the last width. weight / bias are f32 in `mem`, copied.
 * stages == NULL with truncate_dim == 0 removes the head. Every check runs before anything changes: a refused call
 * leaves the encoder as it was. vr_encoder_load resets the head. The reranker never has one. */
#define VR_HEAD_DENSE 0      /* y = act(W x + b): weight [out_dim, in_dim] row-major, bias [out_dim] or NULL */
#define VR_HEAD_LAYERNORM 1  /* y = (x - mean) / sqrt(var + eps) * weight + bias over in_dim (= out_dim) units; bias may be NULL */
#define VR_ACT_IDENTITY 0
#define VR_ACT_TANH 1
typedef struct vr_head_stage {
  int32_t struct_size, kind, in_dim, out_dim, activation;
  float eps;
  const float* weight;
  const float* bias;
} vr_head_stage;
int vr_encoder_set_head(vr_engine* e, const vr_head_stage* stages, int32_t n_stages, int32_t truncate_dim, int mem);

/* ids: concatenated WordPiece ids of n_seq sequences ([CLS] ... [SEP] already added, truncated
 * to max_pos by the tokenizer); offsets: n_seq+1 int32, offsets[0] = 0. Both in `mem`.
 * out: n_seq x W f32 sentence embeddings in `out_mem`, W the encoder's output width (desc.hidden unless
 * vr_encoder_set_head changed it). */
int vr_encode(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq, int mem,
              float* out, int out_mem);

/* vr_encode with one output row per token SPAN instead of per sequence (late chunking: a document goes through the
 * encoder once and each of its chunks is pooled from its own tokens' final hidden states).
 *   span_off  n_seq + 1 int32, starts at 0, never decreases: sequence i owns spans span_off[i] .. span_off[i+1]
 *             (possibly none: such a sequence only provides context)
 *   span_tok  2 int32 per span, (begin, end): token positions inside the span's own sequence,
 *             0 <= begin < end <= len. Spans of a sequence may overlap, repeat and come in any order.
 * ids / offsets / span_off / span_tok in `mem`. out: span_off[n_seq] x W f32 in `out_mem` (W: the encoder's output
 * width, H without a head); row s is the mean over t in [begin, end) of the final hidden state of token t, summed in
 * token order, then (desc.normalize) divided by max(|x|, 1e-12) — with a head (vr_encoder_set_head) the mean goes
 * through its stages first and is cut last. desc.pooling is ignored: the forward pass runs as a mean-pooled model's
 * does, so one span [0, len) on a mean-pooled model gives vr_encode's row bit for bit. Host arrays are checked before
 * any work is queued; vr_last_error names the offending sequence and span. No spans, or n_seq <= 0: returns 0 and
 * writes nothing. */
int vr_encode_spans(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq,
                    const int32_t* span_off, const int32_t* span_tok, int mem,
                    float* out, int out_mem);

/* Semantic chunking: chunk boundaries AND the late-chunked vectors of the resulting chunks from one forward pass.
 * A sequence carries m >= 0 UNITS (sentence-sized token spans), given as vr_encode_spans gives spans (unit_off, unit_tok)
 * but in order and never overlapping: 0 <= begin_r < end_r <= len and begin_{r+1} >= end_r; at most 2048 per sequence.
 * Tokens of no unit only provide context. Per sequence, x_t the final hidden row of token t (vr_encode_spans' rows):
 *   1. S_r = sum of x_t over unit r, f32, token order; n_r = end_r - begin_r
 *   2. C_r = sum of S_j, j = max(0, r - buffer) .. min(m - 1, r + buffer), unit order
 *   3. d_r = 1 - (C_r . C_{r+1}) / max(|C_r| |C_{r+1}|, 1e-12), r = 0 .. m - 2, every sum in a fixed order
 *   4. B = ceil(break_permille (m - 1) / 1000) in integers; rank(r) = the gaps r' with d_r' > d_r, or d_r' == d_r and
 *      r' < r (f32 compares on the stored values); gap r is a CANDIDATE iff rank(r) < B and d_r >= min_distance
 *   5. the walk, left to right, acc = n_0: the chunk is closed behind unit r iff (candidate(r) and acc >= min_tokens)
 *      or acc + n_{r+1} > max_tokens; then acc = n_{r+1}, otherwise acc += n_{r+1}. (A unit above max_tokens is a chunk
 *      of its own; a sequence's last chunk may be below min_tokens; a chunk never crosses a sequence.)
 *   6. a chunk's row: (sum of S_r over its units, unit order) / (sum of n_r), finished as vr_encode_spans finishes a span
 *      mean (head stages, normalize, truncate_dim) — a chunk of one unit is that span's row bit for bit.
 * params: buffer 0..3, break_permille 0..1000, 0 <= min_tokens <= max_tokens, max_tokens >= 1, min_distance any number
 * (above 2 no gap is a candidate). ids / offsets / unit_off / unit_tok in `mem`; the three output arrays in `out_mem`:
 *   out_unit_start  one int32 per unit: 1 where the unit begins a chunk
 *   out_gap_dist    one f32 per unit: d_r, and 0 for a sequence's last unit
 *   out_rows        *n_chunks x W f32 in chunk order (sequence by sequence); capacity: one row per unit
 *   n_chunks        host memory always; the call returns with the stream drained
 * Host arrays and params are checked before any work is queued; vr_last_error names the offending sequence and unit, and
 * a refused call leaves the engine as it was. No units, or n_seq <= 0: returns 0 with *n_chunks = 0, writes nothing else. */
typedef struct vr_semantic_params {
  int32_t struct_size, buffer, break_permille, min_tokens, max_tokens;
  float min_distance;
} vr_semantic_params;
int vr_encode_semantic(vr_engine* e, const int32_t* ids, const int32_t* offsets, int32_t n_seq,
                       const int32_t* unit_off, const int32_t* unit_tok, int mem, const vr_semantic_params* params,
                       float* out_rows, int32_t* out_unit_start, float* out_gap_dist, int32_t* n_chunks, int out_mem);

/* Host-only WordPiece tokenizer (no engine, no GPU): the tokenise step of SentenceTransformer.encode
 * (embedding.py:40,68-73 -> [EXT] HF tokenizers: BertNormalizer, BertPreTokenizer, WordPiece,
 * "[CLS] $A [SEP]", right truncation — SURVEY.md §8 a4 step 2), producing the ids / offsets vr_encode
 * and vr_index_batch take.
 *   vocab_tokens   n_vocab NUL-terminated UTF-8 strings, id = index (vocab.txt line order); must
 *                  contain [UNK], [CLS], [SEP]
 *   lowercase      do_lower_case; strip_accents: 0 / 1, or -1 = follow lowercase (the HF default)
 *   texts[i]       text_lens[i] bytes of UTF-8 (malformed bytes are dropped like U+FFFD)
 *   max_len        longest sequence including [CLS] and [SEP] (max_seq_length)
 *   out_offsets    n_texts + 1; out_ids: at most `capacity` ids written; *needed: total count
 * Returns -2 (offsets and *needed valid) when the buffer is too small. Thread-safe: the tokenizer
 * object is read-only after creation. */
typedef struct vr_wordpiece vr_wordpiece;
int vr_wordpiece_create(const char* const* vocab_tokens, int32_t n_vocab, int32_t lowercase, int32_t strip_accents,
                        int32_t handle_chinese_chars, int32_t clean_text, vr_wordpiece** out);
/* The same tokenizer with the three specials by name (MPNet's WordPiece wraps a sequence in <s> ... </s> and keeps
 * [UNK] as the model's unknown token): cls_token A sep_token, unknown words become unk_token; all three must be in the
 * vocabulary. vr_wordpiece_create is this with "[CLS]", "[SEP]", "[UNK]". With other names than [CLS] / [SEP]
 * vr_wordpiece_encode_pairs is refused: such models pair with another template. */
int vr_wordpiece_create_specials(const char* const* vocab_tokens, int32_t n_vocab, int32_t lowercase, int32_t strip_accents,
                                 int32_t handle_chinese_chars, int32_t clean_text,
                                 const char* cls_token, const char* sep_token, const char* unk_token, vr_wordpiece** out);
void vr_wordpiece_destroy(vr_wordpiece* t);
int vr_wordpiece_encode(const vr_wordpiece* t, const char* const* texts, const int64_t* text_lens, int64_t n_texts,
                        int32_t max_len, int64_t* out_offsets, int32_t* out_ids, int64_t capacity, int64_t* needed);

/* Text PAIRS for a cross-encoder: sequence i is [CLS] A_i [SEP] B_i [SEP] with A_i / B_i tokenised as above and
 * truncated the way HF tokenizers' TruncationStrategy.LongestFirst does to max_len ids including the 3 specials
 * (the shorter side keeps what it can up to half, the longer side the rest). out_seg_b[i] (n entries, may be NULL) is
 * the index inside sequence i of its first segment-B (token type 1) id: the one after the first [SEP]. Each distinct
 * A text is tokenised once per call. out_offsets, out_ids, capacity, *needed and the -2 return as vr_wordpiece_encode;
 * max_len >= 3. */
int vr_wordpiece_encode_pairs(const vr_wordpiece* t, const char* const* a_texts, const int64_t* a_lens,
                              const char* const* b_texts, const int64_t* b_lens, int64_t n, int32_t max_len,
                              int64_t* out_offsets, int32_t* out_ids, int32_t* out_seg_b, int64_t capacity,
                              int64_t* needed);

/* Host-only SentencePiece Unigram tokenizer (XLM-RoBERTa: multilingual-e5, bge-reranker), matching HF tokenizers as an
 * XLM-R tokenizer.json configures it:
 *   1. added tokens matched in the raw text (leftmost-longest; flags VR_ADDED_LSTRIP / _RSTRIP / _SINGLE_WORD as HF
 *      honours them), the pieces between them tokenised separately;
 *   2. the Precompiled normalizer: `charsmap` (the sentencepiece precompiled_charsmap bytes: a darts-clone trie and
 *      its replacement strings) applied per extended grapheme cluster; charsmap_len 0 = no normalizer;
 *   3. replace_spaces != 0: runs of two or more ' ' become one (Replace(" {2,}", " "));
 *   4. pre_tokenizer VR_UNIGRAM_PRE_METASPACE (Metaspace "▁") or VR_UNIGRAM_PRE_WHITESPACE_METASPACE
 *      (Sequence[WhitespaceSplit, Metaspace]), prepend_scheme VR_PREPEND_ALWAYS / _FIRST / _NEVER;
 *   5. Unigram Viterbi over pieces[n_pieces] (NUL-terminated UTF-8, id = index) with f64 scores; characters no piece
 *      covers become unk_id, consecutive ones fused;
 *   6. bos A eos (single), bos A eos eos B eos (pair); truncation as vr_wordpiece_*, with 2 / 4 specials.
 *      bos_id -1 (a T5 tokenizer, template "$A </s>"): A eos, right truncation keeps the eos (max_len - 1 ids of A);
 *      vr_unigram_encode_pairs is refused for such a tokenizer.
 * added[n_added] / added_ids / added_flags: the added tokens (NUL-terminated UTF-8 content, id, flags). Malformed
 * UTF-8 bytes become U+FFFD, as in vr_wordpiece_encode. Read-only after creation and thread-safe. */
typedef struct vr_unigram vr_unigram;
#define VR_UNIGRAM_PRE_METASPACE 0
#define VR_UNIGRAM_PRE_WHITESPACE_METASPACE 1
#define VR_PREPEND_ALWAYS 0
#define VR_PREPEND_FIRST 1
#define VR_PREPEND_NEVER 2
#define VR_ADDED_LSTRIP 1
#define VR_ADDED_RSTRIP 2
#define VR_ADDED_SINGLE_WORD 4
int vr_unigram_create(const char* const* pieces, const double* scores, int32_t n_pieces, int32_t unk_id, int32_t bos_id,
                      int32_t eos_id, const uint8_t* charsmap, int64_t charsmap_len, int32_t replace_spaces,
                      int32_t pre_tokenizer, int32_t prepend_scheme, const char* const* added, const int32_t* added_ids,
                      const int32_t* added_flags, int32_t n_added, vr_unigram** out);
void vr_unigram_destroy(vr_unigram* t);
/* As vr_wordpiece_encode: bos ids... eos, the ids truncated on the right to max_len - 2; max_len >= 2. */
int vr_unigram_encode(const vr_unigram* t, const char* const* texts, const int64_t* text_lens, int64_t n_texts,
                      int32_t max_len, int64_t* out_offsets, int32_t* out_ids, int64_t capacity, int64_t* needed);
/* As vr_wordpiece_encode_pairs: bos A eos eos B eos, truncated LongestFirst to max_len - 4 ids of A and B together;
 * out_seg_b[i] is the index of the first id of B; max_len >= 4. */
int vr_unigram_encode_pairs(const vr_unigram* t, const char* const* a_texts, const int64_t* a_lens,
                            const char* const* b_texts, const int64_t* b_lens, int64_t n, int32_t max_len,
                            int64_t* out_offsets, int32_t* out_ids, int32_t* out_seg_b, int64_t capacity,
                            int64_t* needed);

/* Host-only byte-level BPE tokenizer (ModernBERT: gte-modernbert-base, modernbert-embed-base, gte-reranker-modernbert),
 * matching HF tokenizers as such a tokenizer.json configures it, in its order:
 *   1. added tokens WITHOUT VR_ADDED_NORMALIZED (the specials) matched in the raw text, leftmost-longest, flags as above;
 *   2. the normalizer: NFC (nfc != 0: canonical decomposition, reordering, composition incl. Hangul, the composition
 *      exclusions honoured; tables of the Unicode version named in csrc/bpe_tables.inc) or none;
 *   3. added tokens WITH VR_ADDED_NORMALIZED matched in the normalised text (runs of spaces in ModernBERT's vocabulary);
 *   4. ByteLevel(add_prefix_space=false, use_regex=true): the GPT-2 split
 *      's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+  (case-sensitive), then every byte of
 *      a piece as its code point of the 256-entry byte alphabet;
 *   5. BPE per piece: the lowest-rank merge first, the leftmost among equals; a symbol absent from the vocabulary
 *      becomes unk_id, or is dropped when unk_id is -1;
 *   6. cls ids sep / cls A sep B sep.
 * vocab[n_vocab]: NUL-terminated UTF-8 tokens, the index is the id. merges: n_merges (left, right) token pairs in rank
 * order, merge_left[i] + merge_right[i] must be in the vocabulary. Read-only after creation and thread-safe. */
typedef struct vr_bpe vr_bpe;
#define VR_ADDED_NORMALIZED 8
int vr_bpe_create(const char* const* vocab, int32_t n_vocab, const char* const* merge_left, const char* const* merge_right,
                  int32_t n_merges, int32_t unk_id, int32_t cls_id, int32_t sep_id, int32_t nfc, const char* const* added,
                  const int32_t* added_ids, const int32_t* added_flags, int32_t n_added, vr_bpe** out);
void vr_bpe_destroy(vr_bpe* t);
/* As vr_wordpiece_encode: cls ids... sep, the ids truncated on the right to max_len - 2; max_len >= 2. */
int vr_bpe_encode(const vr_bpe* t, const char* const* texts, const int64_t* text_lens, int64_t n_texts, int32_t max_len,
                  int64_t* out_offsets, int32_t* out_ids, int64_t capacity, int64_t* needed);
/* As vr_wordpiece_encode_pairs: cls A sep B sep, truncated LongestFirst to max_len - 3 ids of A and B together;
 * out_seg_b[i] is the index of the first id of B; max_len >= 3. */
int vr_bpe_encode_pairs(const vr_bpe* t, const char* const* a_texts, const int64_t* a_lens, const char* const* b_texts,
                        const int64_t* b_lens, int64_t n, int32_t max_len, int64_t* out_offsets, int32_t* out_ids,
                        int32_t* out_seg_b, int64_t capacity, int64_t* needed);

/* ---- BM25 document side: replaces SparseTextEmbedding("Qdrant/bm25").embed's token-count / TF
 * weighting (sparse_embedding.py:25,49; scripts/build_sparse_vectors.py:124,170) -- */
/* tok_off: n_docs+1 offsets, tok_ids: abs(murmur3) of each stemmed token in text order (`mem`).
 * Outputs (`mem`), padded layout: document d's distinct term ids, ascending, are
 * out_idx[tok_off[d] .. tok_off[d] + out_cnt[d]) with tf weights (f64, the Python floats the
 * reference passes on) at the same positions of out_val; out_idx/out_val hold tok_off[n_docs]
 * entries. tf = c*(k+1) / (c + k*(1 - b + b*doc_len/avg_len)); fastembed defaults k=1.2 b=0.75
 * avg_len=256. */
int vr_bm25_tf(vr_engine* e, const int64_t* tok_off, const int32_t* tok_ids, int64_t n_docs, int mem,
               double k, double b, double avg_len,
               int32_t* out_cnt, int32_t* out_idx, double* out_val);

/* Host-only text side of fastembed's Bm25 (no engine, no GPU): remove_non_alphanumeric,
 * SimpleTokenizer, stop-word / length filter, Snowball English stemmer, abs(murmur3_x86_32)
 * (SURVEY.md a6/a7 [EXT]). texts[i]: lens[i] bytes of UTF-8. out_off: n+1 offsets; out_ids: the
 * hashed stems of every text in order, at most `cap` written; *out_needed: total count. Returns -2
 * (offsets and *out_needed valid, the leading `cap` ids written) when the buffer is too small: call
 * again with one of *out_needed ids. The same stream serves documents
 * (-> vr_bm25_tf) and queries (Bm25.query_embed = the set of these ids, all values 1.0). */
int vr_bm25_tokenize(const char* const* texts, const int64_t* lens, int64_t n,
                     int64_t* out_off, int32_t* out_ids, int64_t cap, int64_t* out_needed);
/* Snowball English (Porter2) stem of one lower-case UTF-8 word; NUL-terminated into out. */
int vr_porter2_stem(const char* word, int64_t len, char* out, int64_t cap);

/* ---- chunking: replaces ChunkingService.chunk_text (src/voitta/services/chunking.py:33-241,
 * called from services/indexing.py:380,515), the step in front of the path. Host
 * only, one document per host thread. texts[i]: text_lens[i] bytes of UTF-8. chunk_size and
 * chunk_overlap count CHARACTERS (code points, Python's len()). strategy: VR_CHUNK_*; any other
 * value chunks recursively, as the reference does for an unknown name. The call fails when
 * chunk_overlap >= chunk_size AND some text falls through to the fixed-size windows: the
 * reference's window loop never advances there (chunking.py:187) and hangs.
 * The result object holds, until vr_chunks_free:
 *   doc_off   n_texts + 1  chunk index range of each text (an empty / all-blank text has none)
 *   span      2 per chunk  (start_char, end_char) code-point offsets exactly as the reference
 *                          reports them (for overlapped chunks it does not advance start_char)
 *   text_off  n_chunks + 1 byte offsets into `text`, the stripped chunk texts back to back (UTF-8)
 * Chunk.index is the position inside its text's range. */
#define VR_CHUNK_RECURSIVE 0
#define VR_CHUNK_SENTENCE 1
#define VR_CHUNK_FIXED 2
typedef struct vr_chunks vr_chunks;
int vr_chunk_texts(const char* const* texts, const int64_t* text_lens, int64_t n_texts, int32_t chunk_size,
                   int32_t chunk_overlap, int32_t strategy, vr_chunks** out);
int vr_chunks_view(const vr_chunks* c, int64_t* n_chunks, const int64_t** doc_off, const int64_t** span,
                   const int64_t** text_off, const char** text);
void vr_chunks_free(vr_chunks* c);

/* ---- fused indexing step: the three starred calls of IndexingService._index_file_standard
 * (src/voitta/services/indexing.py:527-530,560) — embed_texts, sparse embed_texts, store_chunks —
 * without leaving HBM: encode (vr_encode) -> BM25 tf (vr_bm25_tf) -> store (vr_upsert).
 * wp_ids / wp_off (int32, n+1): WordPiece ids per chunk; bm_ids / bm_off (int64 offsets, n+1):
 * hashed stems per chunk, or both NULL for a dense-only index. Token arrays are in `mem`; the
 * payload columns are host arrays as in vr_upsert. Needs a loaded encoder with hidden == dim. */
int vr_index_batch(vr_engine* e, int64_t n, int mem,
                   const int32_t* wp_ids, const int32_t* wp_off,
                   const int32_t* bm_ids, const int64_t* bm_off,
                   double k, double b, double avg_len,
                   const int32_t* folder_id, const int32_t* index_folder_id,
                   const int64_t* created, const int64_t* modified,
                   int64_t* out_first_row);

/* vr_index_batch for rows that are spans (vr_encode_spans) of n_seq sequences: n must equal span_off[n_seq]; row r gets
 * the dense vector of span r, the BM25 vector of bm_ids / bm_off entry r (n entries, per chunk as above) and payload
 * entry r. */
int vr_index_batch_spans(vr_engine* e, int64_t n, int mem,
                         const int32_t* wp_ids, const int32_t* wp_off, int32_t n_seq,
                         const int32_t* span_off, const int32_t* span_tok,
                         const int32_t* bm_ids, const int64_t* bm_off,
                         double k, double b, double avg_len,
                         const int32_t* folder_id, const int32_t* index_folder_id,
                         const int64_t* created, const int64_t* modified,
                         int64_t* out_first_row);

/* ---- index: replaces VectorStoreService.store_chunks' client.upsert (vector_store.py:291-313)
 * and the Qdrant-side cosine normalisation on insert (SURVEY.md a10 [EXT]). ------------------- */
/* dense   : n x D f32 row-major
 * sp_off  : n+1 CSR offsets, sp_idx/sp_val : BM25 (token id, tf weight); NULL sp_off => rows carry
 *           no sparse vector (vector_store.py:299-300)
 * folder_id / index_folder_id : per-row dictionary ids (NULL => 0)
 * created / modified : per-row epochs or VR_TS_ABSENT (NULL => all absent)
 * out_first_row : rows [first, first+n) were assigned */
int vr_upsert(vr_engine* e, int64_t n, int mem,
              const float* dense,
              const int64_t* sp_off, const int32_t* sp_idx, const float* sp_val,
              const int32_t* folder_id, const int32_t* index_folder_id,
              const int64_t* created, const int64_t* modified,
              int64_t* out_first_row);

/* tombstone rows (host pointer); replaces the filtered client.delete of vector_store.py:340-352,
 * :378-390,:419-431 once the host has resolved the filter to rows. Already-dead rows are ignored;
 * document frequencies and the sparse point count are decremented. */
int vr_delete_rows(vr_engine* e, const int64_t* rows, int64_t n);

/* counters of the two-stage dense search (see VR_ENGINE_NO_PREFILTER) */
#define VR_STAT_TWO_STAGE 0        /* single-query dense searches served by f16 scan + exact re-score */
#define VR_STAT_FALLBACK 1         /* ... of which exceeded the re-score budget and were redone one-stage */
#define VR_STAT_LAST_CANDIDATES 2  /* rows re-scored by the last two-stage search */
#define VR_STAT_BATCHED 3          /* queries served by the batched (integer GEMM) dense search */
#define VR_STAT_BATCH_FALLBACK 4   /* ... of which exceeded their candidate budget and were redone alone */
#define VR_STAT_BATCH_CANDIDATES 6 /* rows re-scored exactly by the batched search, summed over its queries */
#define VR_STAT_SPARSE_GROUPED 7    /* sparse queries served by the grouped batch scan (groups of queries share a block per segment) */
#define VR_STAT_SPARSE_GROUP_REDO 8 /* queries that scan gave up (a candidate region overflowed) and the per-query kernels redid */
#define VR_STAT_SPARSE_GROUP_CANDIDATES 9 /* candidate keys the grouped scan's selections ranked (counted when the NEXT batch starts) */
#define VR_STAT_GENERATION 5       /* bumped whenever row numbers change meaning (vr_compact, vr_load): a host
                                      table keyed by row is valid for the generation it was built against */
int vr_stats(vr_engine* e, int32_t which, int64_t* out);

/* n_rows = rows ever assigned, n_live = not tombstoned (get_collection_info, vector_store.py:699-710) */
int vr_count(vr_engine* e, int64_t* n_rows, int64_t* n_live);

/* read back stored (normalised) dense rows — scroll(with_vectors=True) of
 * scripts/build_sparse_vectors.py:140-146. out: n x D f32 (host). */
int vr_get_dense(vr_engine* e, const int64_t* rows, int64_t n, float* out);

/* document frequency of token ids and the sparse point count N (Qdrant Modifier.IDF statistics,
 * vector_store.py:95-99). ids/out_df are host pointers. */
int vr_sparse_stats(vr_engine* e, const int32_t* ids, int32_t n, int32_t* out_df, int64_t* out_n_points);

/* ---- search: replaces client.query_points (vector_store.py:612-617, :640-656) ------------- */
/* q : nq x D f32 (`mem`); results (host): rows[nq*k] (-1 padded), scores[nq*k], counts[nq].
 * Exact f32 brute force over live rows that pass `filter` (NULL = none), score = k-ordered f32
 * fma chain of q_hat . x_hat, ties broken by the lower row id.
 * More than 16 queries at once (BASELINE configs[4]: 1k batched queries) are served by an int8
 * matrix-core GEMM over the shadow corpus with certain error bounds, followed by an exact re-score of
 * the candidates (csrc/batch.hip): same results, bit for bit, at a small fraction of nq single searches. */
int vr_search_dense(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k,
                    const vr_filter* filter,
                    int64_t* rows, float* scores, int32_t* counts);

/* The same search with the results left as packed ranking keys, nq x k uint64 in `keys_mem` memory (host or
 * device): key = (order-preserving bits of the f32 score << 32) | (0xFFFFFFFF - row), descending, 0 = no result.
 *   score bits: u = key >> 32;  f32 bits = (u & 0x80000000) ? u ^ 0x80000000 : ~u;   row = 0xFFFFFFFF - (key & 0xFFFFFFFF)
 * A sharded caller (voitta_rag_amd/sharded.py) hands the device array of a whole query batch straight to its
 * RCCL all_gather — the per-shard top-k merge of SURVEY.md §8e — without a host round trip per query. */
int vr_search_dense_keys(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k, const vr_filter* filter,
                         uint64_t* keys, int keys_mem);

/* one sparse query (host pointers): score(d) = sum_t (q_t * idf(t)) * d_t over shared terms in
 * ascending token-id order, idf(t) = ln(1 + (N - df_t + 0.5)/(df_t + 0.5)); rows sharing no
 * term are not returned. */
int vr_search_sparse(vr_engine* e, const int32_t* q_idx, const float* q_val, int32_t nnz,
                     int32_t k, int32_t weights_given, const vr_filter* filter,
                     int64_t* rows, float* scores, int32_t* count);
/* weights_given != 0: q_val[t] already is q_t * idf(t) and the engine applies no IDF. Used when
 * the corpus is sharded over several engines (one per GPU): the caller all-reduces the document
 * frequencies of the query terms (vr_sparse_stats) and computes idf with vr_idf, so that every
 * shard scores with the collection-wide statistic. */
float vr_idf(int64_t n_points, int32_t df);

/* ---- measurement: HIP-event timing of the engine's own kernels on its stream ---------------- */
#define VR_PROF_GEMM 0         /* encoder GEMMs; work = FLOP (2*M*N*K) */
#define VR_PROF_ATTENTION 1    /* work = FLOP (4 * H * sum len^2) */
#define VR_PROF_DENSE_SCAN 2   /* work = bytes (N*D*4 + masks + scores) */
#define VR_PROF_SPARSE_SCAN 3  /* work = bytes (4 per stored id + 5 per row) */
#define VR_PROF_BATCH_SCAN 4   /* batched dense search, both integer-GEMM passes; work = operations (2*N*D*Q) */
/* enable != 0 clears earlier records and starts recording one event pair per launch */
int vr_profile(vr_engine* e, int enable);
int vr_profile_read(vr_engine* e, int kernel_class, double* total_ms, int64_t* launches,
                    double* total_work);

/* hybrid: restates VectorStoreService._hybrid_search (vector_store.py:621-697): dense and sparse
 * top-(3*limit), min-max normalisation, (1-w)*d + w*s over the id union, top-`limit`.
 * out_scores are the fused scores as f64 (Python floats in the reference, :680,:694).
 * out_from_dense[i] = 1 when the row was in the dense list (:682-685). */
int vr_search_hybrid(vr_engine* e, const float* q, int mem,
                     const int32_t* q_idx, const float* q_val, int32_t nnz,
                     int32_t limit, double sparse_weight, int32_t fusion,
                     const vr_filter* filter,
                     int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count);

/* ---- many queries per call (BASELINE configs[4]: 1k batched hybrid queries; the caller that would batch is the MCP
 * search tool under load, mcp_server.py:469-485). The sparse queries of a batch are one CSR: query i's terms are
 * q_idx / q_val [q_off[i], q_off[i + 1]) (host pointers). Results are, bit for bit, those of nq single calls. ---- */

/* nq sparse queries (vector_store.py:647-656, once per query): rows[nq*k] (-1 padded), scores[nq*k], counts[nq].
 * Queries of up to 32 distinct terms share ONE launch over the inverted index (csrc/invert.hip: grid = segment
 * share x query); longer ones, k > 64 and collections kept on the forward scan are served one by one. */
int vr_search_sparse_batch(vr_engine* e, const int64_t* q_off, const int32_t* q_idx, const float* q_val, int32_t nq,
                           int32_t k, int32_t weights_given, const vr_filter* filter,
                           int64_t* rows, float* scores, int32_t* counts);

/* nq hybrid queries (_hybrid_search, vector_store.py:621-697, once per query): the dense legs as ONE batched dense
 * search, the sparse legs as ONE batched sparse search beside it (second stream), the fusion of every query on the
 * host threads. q: nq x D f32 (`mem`); sq_off may be NULL (no query has sparse terms).
 * out_rows / out_scores / out_from_dense: nq x limit (entries beyond out_counts[i] are unspecified). */
int vr_search_hybrid_batch(vr_engine* e, const float* q, int32_t nq, int mem,
                           const int64_t* sq_off, const int32_t* sq_idx, const float* sq_val,
                           int32_t limit, double sparse_weight, int32_t fusion, const vr_filter* filter,
                           int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts);

/* Filtered batches: every query with its own filter (the MCP search tool under multi-user load: include_folders from the
 * user's active folders, exclude_folders, dates, limit and sparse_weight per call, mcp_server.py:374-461). Query i uses
 * filters[filter_of_query[i]], or none when filter_of_query[i] is -1; every distinct entry is a CLASS. Row i is, bit for
 * bit, what the single call with query i's own arguments returns. The batched dense scan reads one bit plane per class
 * (csrc/filter.hip) instead of one shared mask, so a batch of many classes still scans the corpus once; the grouped
 * sparse scan forms its groups of queries of one class, each reading that class's plane (collections of >= 128 index
 * segments; otherwise, and for what the batched scans do not take, class by class on a byte mask). One class takes the
 * unfiltered-batch path (vr_search_dense / vr_search_hybrid_batch) unchanged. VR_CLASS_PLANE_MIB (default 256) bounds
 * the planes of one scan; a batch needing more runs in slices of classes. 
 * filter_of_query, every filter's struct_size and n_must_folder_sets, k and every limits[i] (1..341) are checked before
 * any device work. */

/* nq dense queries, k each: rows[nq*k] (-1 padded), scores[nq*k], counts[nq] as vr_search_dense(q_i, k, filter_i). */
int vr_search_dense_multi(vr_engine* e, const float* q, int32_t nq, int mem, int32_t k,
                          const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query,
                          int64_t* rows, float* scores, int32_t* counts);

/* nq hybrid queries as vr_search_hybrid(q_i, sparse_i, limits[i], sparse_weights[i], fusion, filter_i); sq_off may be
 * NULL. out_rows / out_scores / out_from_dense: nq x out_stride (out_stride >= every limit; entries beyond out_counts[i]
 * are unspecified). */
int vr_search_hybrid_batch_multi(vr_engine* e, const float* q, int32_t nq, int mem,
                                 const int64_t* sq_off, const int32_t* sq_idx, const float* sq_val,
                                 const int32_t* limits, const double* sparse_weights, int32_t fusion,
                                 const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query,
                                 int32_t out_stride, int64_t* out_rows, double* out_scores,
                                 int32_t* out_from_dense, int32_t* out_counts);

/* Both legs of nq hybrid queries as packed ranking keys (see vr_search_dense_keys), for a sharded caller: keys is
 * [nq][2][k] uint64 in `keys_mem` memory — per query its dense list, then its sparse list. weights_given as in
 * vr_search_sparse. The caller all-gathers the array, merges with vr_merge_keys and fuses with vr_fuse_batch
 * (fusion runs on MERGED lists, never per shard: vector_store.py:659-689). */
int vr_search_hybrid_keys(vr_engine* e, const float* q, int32_t nq, int mem,
                          const int64_t* sq_off, const int32_t* sq_idx, const float* sq_val,
                          int32_t k, int32_t weights_given, const vr_filter* filter, uint64_t* keys, int keys_mem);

/* The per-shard top-k merge of SURVEY.md §8e on the engine's own kernel: parts is [n_parts][n_lists][k] keys (`mem`:
 * the tensor an RCCL all_gather filled, or a host array), part p holding shard p's lists. Every list is merged over
 * the parts — score descending, then lower local row, then lower part, i.e. ascending global id row * n_parts + p —
 * into out_ids (global ids, -1 padded), out_scores and out_counts, host arrays [n_lists][k] / [n_lists].
 * n_parts * k <= 4096. */
int vr_merge_keys(vr_engine* e, const uint64_t* parts, int32_t n_parts, int32_t n_lists, int32_t k, int mem,
                  int64_t* out_ids, float* out_scores, int32_t* out_counts);

/* MMR selection over candidate lists of stored rows. List i is rows[list_off[i] .. list_off[i+1]) with
 * relevance[...] (f64, first-stage order), diversity[i] in [0, 1], limits[i] >= 0; list length <= 1024.
 * out_pos: n_lists x out_stride (out_stride >= every limit), positions into list i in selection order;
 * out_counts[i] = min(limits[i], length). All arrays are host arrays. `generation` is the VR_STAT_GENERATION the
 * rows were read under: if the index has been renumbered since, nothing runs and VR_STALE_GENERATION (> 0) is
 * returned. Rows outside [0, n_rows) and bad arguments are errors (< 0), checked before any device work.
 * Selection: step 1 picks the largest (1 - d) * rel_i, every later step the largest (1 - d) * rel_i - d * (double) m_i,
 * m_i the f32 maximum of sim(i, s) over the picks s so far, sim the f32 dense score of one stored row against another;
 * f64 operations rounded one at a time, ties to the lower position. Tombstoned rows are allowed. */
#define VR_STALE_GENERATION 1
int vr_mmr_select(vr_engine* e, int32_t n_lists, const int64_t* list_off, const int64_t* rows,
                  const double* relevance, const double* diversity, const int32_t* limits, int64_t generation,
                  int32_t out_stride, int32_t* out_pos, int32_t* out_counts);

/* The fusion arithmetic for nq pairs of lists at once, on the host threads (vector_store.py:659-697 per query; the
 * last step of a batched or sharded hybrid search). d_* / s_*: [nq][k] with counts [nq] (s_* may be NULL);
 * out_*: [nq][limit], out_counts [nq]. fusion: VR_FUSION_*; json_scores as in vr_fuse_minmax. */
int vr_fuse_batch(const int64_t* d_rows, const float* d_scores, const int32_t* d_counts,
                  const int64_t* s_rows, const float* s_scores, const int32_t* s_counts,
                  int32_t nq, int32_t k, int32_t limit, double sparse_weight, int32_t fusion, int32_t json_scores,
                  int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts);

/* ---- collection-wide document frequencies on a sharded corpus ("one all-reduce (sum) of df deltas
 * after each upsert/delete batch"; Qdrant's Modifier.IDF statistic is collection-wide, vector_store.py:95-99).
 * Every shard's table holds the statistic of ALL shards: after a shard stored (or before it deletes) rows, it exports
 * their term ids, the shards exchange them (all_gather) and each applies the OTHERS' ids. A query then needs no
 * exchange of statistics: one collective (the result merge) per hybrid query. -------------------------------------- */

/* Term ids of the listed rows' sparse vectors in a fixed-stride layout: out[i * stride + j], -1 where row i has no
 * j-th entry, is tombstoned or carries no sparse vector; out (`mem`, room for cap ids) may be NULL to ask for the
 * stride alone. *stride = the widest stored sparse row; *n_points = listed rows that are live and carry a sparse
 * vector. rows is a host array. */
int vr_sparse_row_ids(vr_engine* e, const int64_t* rows, int64_t n, int32_t* out, int64_t cap, int mem,
                      int32_t* stride, int64_t* n_points);
/* df[id] += sign for every id >= 0 of ids (`mem`), sparse point count += sign * n_points: the statistics of rows
 * that live on other shards. sign = +1 (stored there) or -1 (deleted there). */
int vr_df_apply(vr_engine* e, const int32_t* ids, int64_t n_ids, int mem, int64_t n_points, int32_t sign);

/* A question as TEXT, answered in one call: the three calls of the MCP search tool (mcp_server.py:469-485:
 * embedding_service.embed_query, sparse_service.embed_query, vector_store.search) without the trips through the host
 * language between them. dense_text: the query as the encoder sees it (with its "query: " prefix for e5 models,
 * embedding.py:82-83), tokenised by `tokenizer` ([CLS] .. [SEP], truncated to max_len); sparse_text: the raw query for
 * the BM25 side (Bm25.query_embed: the set of its hashed stems, every value 1.0), or NULL / length 0 for a dense-only
 * search. Branch selection as VectorStoreService.search (vector_store.py:560-619): hybrid (prefetch 3 x limit, fusion)
 * when a stem survives, else the dense top-`limit` with its cosine scores widened to f64 (the caller applies the
 * REST/JSON transport). *out_hybrid says which ran. Needs a loaded encoder with hidden == dim. */
int vr_query_text(vr_engine* e, const vr_wordpiece* tokenizer, const char* dense_text, int64_t dense_len,
                  const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit, double sparse_weight,
                  int32_t fusion, const vr_filter* filter,
                  int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count, int32_t* out_hybrid);

/* n questions as TEXT in one call, each with its own filter, limit and sparse weight: row i is what vr_query_text
 * returns for question i (dense_texts[i], sparse_texts[i], limits[i], sparse_weights[i], fusion,
 * filters[filter_of_query[i]] or none for -1), in branch and score alike. sparse_texts may be NULL, and so may an
 * entry of it (length 0 likewise): no sparse leg for that question. One forward pass over all n questions (the
 * embeddings are those vr_encode gives for the same tokenised list) whose rows stay in device memory and feed the
 * filtered batch searches of vr_search_hybrid_batch_multi (questions with a stem) and vr_search_dense_multi (the
 * others). out_rows / out_scores / out_from_dense: n x out_stride (out_stride >= every limit; entries beyond
 * out_counts[i] are unspecified); out_hybrid[n] (may be NULL) says which branch ran; out_embeddings (n x hidden f32,
 * host; may be NULL) receives the embeddings. Arguments are checked before any device work; n = 0 does nothing. */
int vr_query_text_batch(vr_engine* e, const vr_wordpiece* tokenizer, int32_t n, const char* const* dense_texts,
                        const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                        int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                        const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query, int32_t out_stride,
                        int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_counts,
                        int32_t* out_hybrid, float* out_embeddings);

/* vr_query_text and vr_query_text_batch with a Unigram tokenizer (XLM-R: <s> .. </s>): the same pipeline, the same
 * arguments and results. */
int vr_query_text_unigram(vr_engine* e, const vr_unigram* tokenizer, const char* dense_text, int64_t dense_len,
                          const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit,
                          double sparse_weight, int32_t fusion, const vr_filter* filter,
                          int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count,
                          int32_t* out_hybrid);
/* ... and with a byte-level BPE tokenizer (vr_bpe_encode). */
int vr_query_text_bpe(vr_engine* e, const vr_bpe* tokenizer, const char* dense_text, int64_t dense_len,
                          const char* sparse_text, int64_t sparse_len, int32_t max_len, int32_t limit,
                          double sparse_weight, int32_t fusion, const vr_filter* filter,
                          int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count,
                          int32_t* out_hybrid);
int vr_query_text_batch_unigram(vr_engine* e, const vr_unigram* tokenizer, int32_t n, const char* const* dense_texts,
                                const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                                int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                                const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query,
                                int32_t out_stride, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                                int32_t* out_counts, int32_t* out_hybrid, float* out_embeddings);
/* ... and with a byte-level BPE tokenizer (vr_bpe_encode). */
int vr_query_text_batch_bpe(vr_engine* e, const vr_bpe* tokenizer, int32_t n, const char* const* dense_texts,
                                const int64_t* dense_lens, const char* const* sparse_texts, const int64_t* sparse_lens,
                                int32_t max_len, const int32_t* limits, const double* sparse_weights, int32_t fusion,
                                const vr_filter* filters, int32_t n_filters, const int32_t* filter_of_query,
                                int32_t out_stride, int64_t* out_rows, double* out_scores, int32_t* out_from_dense,
                                int32_t* out_counts, int32_t* out_hybrid, float* out_embeddings);

/* ---- Cross-encoder reranking: a second BERT model in the engine, beside the embedder -------------------------------
 * vr_reranker_load: a BertForSequenceClassification with one label (cross-encoder/ms-marco-MiniLM-L-6-v2 and the
 * like). desc / tensors / mem as vr_encoder_load, followed by 4 more tensors: pooler.dense.weight [H,H],
 * pooler.dense.bias [H], classifier.weight [1,H], classifier.bias [1] (5 + 16 L + 4 in all). desc->pooling must be
 * VR_POOL_CLS and desc->normalize 0; position VR_POS_LEARNED and ffn VR_FFN_GELU (a rotary or gated description is
 * refused and a loaded reranker stays as it is); any precision; type_vocab >= 1; H need not equal the engine's dim. An XLM-R
 * cross-encoder (XLMRobertaForSequenceClassification: out_proj(tanh(dense(h_<s>)))) loads the same way, its
 * classifier.dense / classifier.out_proj as the four head tensors, type_vocab 1, and its position table from row
 * pad_token_id + 1 on (max_pos = max_position_embeddings - pad_token_id - 1). The model gets
 * its own weights, workspace and graph cache, is replaced by the next load and freed with the engine; loading it never
 * touches the embedder.
 * A ModernBERT cross-encoder (ModernBertForSequenceClassification with one label: gte-reranker-modernbert-base): a
 * description with norm VR_NORM_PRE, position VR_POS_ROTARY and a gated ffn, with window / global_every / both thetas as
 * vr_encoder_load takes them, type_vocab 1, normalize 0, pooling VR_POOL_CLS or VR_POOL_MEAN (config.json's
 * classifier_pooling) over the final norm's rows. Its tensors are vr_encoder_load's 5 + 18 L followed by 6: head.dense.weight
 * [H,H], head.dense.bias [H], head.norm.weight [H], head.norm.bias [H], classifier.weight [1,H], classifier.bias [1]
 * (zeros where the checkpoint has no head.dense.bias or no head.norm.bias; none may be NULL). Its logit is
 * wc . LN(gelu(Wd p + bd)) + bc: p the pooled row, gelu the exact-erf one, LN with the description's eps. Any other
 * mix of norm, window, position and ffn is refused. */
int vr_reranker_load(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors, int32_t n_tensors, int mem);

/* A decoder cross-encoder in the same reranker slot (Qwen3-Reranker-0.6B, one-label Qwen3ForSequenceClassification /
 * Qwen2ForSequenceClassification): the body vr_encoder_load takes under VR_NORM_PRE_RMS_ROTARY — position
 * VR_POS_ROTARY, a gated ffn, causal 0 or 1, head_dim and qk_norm as vr_encoder_load takes them (vr_bert_desc_v2 / _v3),
 * type_vocab 1, any precision — with pooling VR_POOL_LAST and normalize 0. Its tensors are vr_encoder_load's 5 + 18 L
 * (5 + 20 L with qk_norm) followed by ONE head tensor, score.weight [1, H] f32, never NULL. The logit of a pair is
 * score.weight . N_f(h_last): h_last the residual row of the pair's LAST token, N_f the final RMSNorm; no bias.
 * Qwen3-Reranker's published score, softmax over (lm_head[no] . h, lm_head[yes] . h) taken at "yes", is the sigmoid of
 * that logit with score.weight = lm_head[yes] - lm_head[no], which the caller computes (embed_tokens where tied).
 * Everything outside this description is refused with the field and its value named; a refused load leaves a loaded
 * reranker as it was. vr_rerank, replacement by the next load of either kind and freeing are vr_reranker_load's;
 * vr_reranker_load itself keeps refusing this norm.
 * The prompt is the caller's job: the ids of a pair are prefix + body + suffix of the model's chat template (system
 * instruction, "<Instruct>: .. <Query>: .. <Document>: ..", the assistant turn with its empty think block), so that
 * the last token is the one the model answers "yes" or "no" behind. Only the last row of each pair is computed behind
 * the last layer's attention (the output projection, the FFN and the final norm run on n_seq rows). */
int vr_reranker_load_decoder(vr_engine* e, const vr_bert_desc* desc, const void* const* tensors, int32_t n_tensors, int mem);

/* One logit per (question, passage) pair: logit = wc . tanh(Wp h_CLS + bp) + bc, h_CLS the last hidden state of the
 * pair's [CLS] token (a ModernBERT cross-encoder: its own head, see vr_reranker_load). ids / offsets as vr_encode (pair sequences, e.g. from vr_wordpiece_encode_pairs); seg_b[n_seq]
 * int32: tokens at positions >= seg_b[i] of sequence i are segment B (token type 1), 1 <= seg_b[i] <= its length. A
 * model with one token type (type_vocab 1, XLM-R) has no segment B: seg_b may be NULL and is ignored. A decoder
 * cross-encoder (vr_reranker_load_decoder) has one token type too; its logit is score.weight . N_f(h_last). All three in
 * `mem`; out_logits: n_seq f32 in `out_mem`. The head runs in f32 whatever the precision, in a fixed order:
 * the same input gives the same bits. Arguments are checked before any device work. */
int vr_rerank(vr_engine* e, const int32_t* ids, const int32_t* offsets, const int32_t* seg_b, int32_t n_seq, int mem,
              float* out_logits, int out_mem);

/* The same from text: n_queries questions, question q paired with passages [cand_off[q], cand_off[q+1]) (cand_off:
 * n_queries + 1 int64, cand_off[0] = 0, non-decreasing; a question may have none). Pairs are tokenised by `tokenizer`
 * (vr_wordpiece_encode_pairs, max_len) on the host threads and scored in ONE forward pass; out_logits (host) receives
 * cand_off[n_queries] logits in pair order, each equal to what vr_rerank gives for the same ids. */
int vr_rerank_text(vr_engine* e, const vr_wordpiece* tokenizer, int32_t n_queries, const char* const* queries,
                   const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                   const int64_t* passage_lens, int32_t max_len, float* out_logits);
/* The same with a Unigram tokenizer (vr_unigram_encode_pairs, max_len >= 4). */
int vr_rerank_text_unigram(vr_engine* e, const vr_unigram* tokenizer, int32_t n_queries, const char* const* queries,
                           const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                           const int64_t* passage_lens, int32_t max_len, float* out_logits);
/* The same with a byte-level BPE tokenizer (vr_bpe_encode_pairs, max_len >= 3). */
int vr_rerank_text_bpe(vr_engine* e, const vr_bpe* tokenizer, int32_t n_queries, const char* const* queries,
                       const int64_t* query_lens, const int64_t* cand_off, const char* const* passages,
                       const int64_t* passage_lens, int32_t max_len, float* out_logits);

/* Persistence. The reference's index survives a restart in Qdrant's volume
 * (docker-compose.yml:8-9; VectorStoreService._ensure_collection re-attaches, vector_store.py:75-115).
 * vr_save writes everything the device owns — tiled dense corpus, payload columns, tombstones,
 * SELL sparse index, document-frequency table — to ONE file (written to path + ".tmp", then renamed
 * over `path`); vr_load restores it into an EMPTY engine of the same dimension and rebuilds the
 * search shadow. Row numbers, scores and rankings after a load are identical to those before the
 * save. The file is checksummed; a truncated or corrupt file is refused. Payload text, point ids
 * and the folder dictionaries belong to the host (voitta_rag_amd/vector_store.py saves them beside it). */
int vr_save(vr_engine* e, const char* path);

/* Reclaim tombstoned rows. The reference deletes points in place while it
 * serves (watcher deletes, re-index = delete + insert, orphan purge: services/indexing.py:281-288,
 * 696-721,886-901, watcher.py:149-171) and Qdrant's optimiser compacts segments in the background;
 * here vr_delete_rows leaves tombstones and this call rebuilds every table without them.
 * Surviving rows keep their relative order and are renumbered 0..n_live-1:
 *   new_row_of_old  host int64[rows before the call] (may be NULL): new row, or -1 for a dropped row
 *   n_rows_after    rows (= live rows) after the call
 * Scores and rankings are unchanged (document frequencies and the sparse point count never
 * included deleted rows). The compacted tables are built beside the live ones; searches keep running
 * and only wait for the final exchange of pointers. VR_STAT_GENERATION is bumped by that exchange. */
int vr_compact(vr_engine* e, int64_t* new_row_of_old, int64_t* n_rows_after);
int vr_load(vr_engine* e, const char* path);

/* The fusion arithmetic alone (host, no GPU): what vector_store.py:659-697 does to two result
 * lists. Exposed so the reference's own two-list code path can be checked in isolation.
 * json_scores != 0 reproduces the REST transport of the reference (f32 score -> shortest decimal
 * -> Python float) instead of exact f32->f64 widening. */
int vr_fuse_minmax(const int64_t* d_rows, const float* d_scores, int32_t nd,
                   const int64_t* s_rows, const float* s_scores, int32_t ns,
                   int32_t limit, double sparse_weight, int32_t json_scores,
                   int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count);

/* Reciprocal-rank fusion of the same two lists (host, no GPU): the arithmetic of vr_search_hybrid's
 * VR_FUSION_RRF mode in isolation. The reference does not fuse this way — its own note says why
 * (vector_store.py:638-639: Qdrant's prefetch + fusion is RRF-only, hence the weighted min-max path) —
 * north_star names it, so it is offered and checked against oracle/fusion.py::rrf_fuse:
 * score(id) = sum over the lists holding id of 1 / (position + 2), position counted from 0 [EXT: the
 * Qdrant server's RRF]; ties in the fused score go to the lower row id. */
int vr_fuse_rrf(const int64_t* d_rows, int32_t nd, const int64_t* s_rows, int32_t ns, int32_t limit,
                int64_t* out_rows, double* out_scores, int32_t* out_from_dense, int32_t* out_count);

#ifdef __cplusplus
}
#endif
#endif /* VOITTA_ENGINE_H */
