// Decode engine: host side of include/tinyllm_engine.h.
//   * page allocator + slot table (slot_table.h: the host mirror of block_table / context_lens), transactional reserve
//     (reference semantics: TinyKvPagedPool / TinyKvPagedCache, src/tiny_llm_ref/paged_kv_cache.py:21-443)
//   * one fused decode step = 5 launches per layer (+ merge when the context is split) + 2 at the end,
//     captured into a hipGraph per (batch, n_splits) and replayed
//   * multi-token prefill on the MFMA W4 GEMM + paged FlashAttention operators of tinyllm_hip.h
#include <dlfcn.h>

#include <cstddef>
#include <cstring>
#include <memory>
#include <type_traits>

#include "decode_linear.h"  // the projection router; with it common.h, engine_kernels.h and the decode matmuls' headers
#include "device_block.h"
#include "engine_layout.h"
#include "step_end.h"  // the three step-end kernels; with it sample.h and logprob.h
#include "dry.h"
#include "lookup.h"
#include "logit_process.h"
#include "truncate.h"
#include "grammar_stack.h"
#include "decode_attention.h"  // the decode attention's launch; with it attn_plan.h and attn_mfma.h
#include "aql.h"
#include "prefix_cache.h"
#include "replay_route.h"
#include "kv_copy.h"
#include "beam.h"
#include "kv_swap.h"
#include "pool.h"
#include "lora.h"
#include "slot_settings.h"
#include "slot_table.h"
#include "stop.h"
#include "stop_set.h"
#include "verify_attn_host.h"  // the launches of the batched verification (their kernels: verify_attn.h, compiled by verify_attn.hip)

namespace tl {

#define TL_HIP(expr)                                                                           \
    do {                                                                                       \
        const hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess) return fail(TL_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

}  // namespace tl

using namespace tl;

// the vocabulary as byte strings and a byte-level automaton over it (grammar.h): device copies for the kernels, host copies for
// validation and tl_engine_grammar_state's walk of a pending token
struct tl_vocab {
    int vocab = 0;
    std::vector<int32_t> offsets;
    std::vector<uint8_t> bytes;
    DeviceBlock mem;
    int32_t *offsets_dev = nullptr;
    uint8_t *bytes_dev = nullptr;
    // the long tokens (more than GR_LONG bytes): their ids, ascending, and per token its number among them
    std::vector<int32_t> long_ids;
    int32_t *long_index_dev = nullptr, *long_ids_dev = nullptr;
};
struct tl_grammar {
    const tl_vocab *vocab = nullptr;
    int n_states = 0, start = 0;
    std::vector<uint16_t> table;  // a regex grammar's
    std::vector<uint8_t> accepting;
    std::vector<int32_t> eos;
    DeviceBlock mem;
    GrammarDev *dev = nullptr;  // what a slot's pointer is poked to
    // a stack grammar (tl_grammar_create_stack): in place of `table`, the two tables in the shape the device holds them (grammar_stack.h)
    bool stack = false;
    int n_pop = 0;
    std::vector<uint32_t> fused;  // [n_states][256] entry | op << 16
    std::vector<uint16_t> pop8;   // [max(n_pop, 1)][8]
    bool is_eos(int token) const { return std::find(eos.begin(), eos.end(), token) != eos.end(); }
    // advance of the definition on a configuration (a regex grammar's: (state, 0, 0)), END = (-1, 0, 0): the device's transition rules
    // (gr_step, grs_step) on the host copies
    GrsConfig advance(GrsConfig c, int token) const {
        const GrsConfig end{GR_END, 0, 0ull};
        if (c.state < 0 || token < 0 || token >= vocab->vocab || is_eos(token)) return end;
        const int b0 = vocab->offsets[token], b1 = vocab->offsets[token + 1];
        if (b1 <= b0) return end;
        for (int k = b0; k < b1; ++k) {
            if (stack) {
                if (!grs_step(fused.data(), pop8.data(), c, vocab->bytes[k])) return end;
            } else {
                const uint32_t to = gr_step(table.data(), (uint32_t)c.state, vocab->bytes[k]);
                if (to == GR_DEAD) return end;
                c.state = (int)to;
            }
        }
        return c;
    }
};

// a stop set (tl_stop_create; stop_set.h builds it, stop.h reads it): the host copy for validation, one device allocation for the kernel
struct tl_stop {
    StopSet set;
    const tl_vocab *vocab = nullptr;  // the vocabulary the text is counted and the strings are matched in (borrowed); may be null for a set of ids
    DeviceBlock mem;
    StopDev *dev = nullptr;  // what a slot's pointer is poked to
};

struct tl_engine {
    tl_engine_config cfg{};
    std::vector<tl_layer_weights> layers;
    tl_w4 embed{}, lm_head{};
    const void *final_norm = nullptr;
    hipStream_t stream = nullptr;
    // the stream the engine created for itself (null: the caller's).  Declared ahead of every DeviceBlock: members go in reverse
    // order, so the stream outlives the memory its work touched
    struct OwnedStream {
        hipStream_t s = nullptr;
        ~OwnedStream() {
            if (s) (void)hipStreamDestroy(s);
        }
    } owned_stream;

    // device memory (one arena for state + activations, one for KV).  Every allocation has its DeviceBlock here (device_block.h); the
    // typed pointers beside them are what the launches read
    DeviceBlock arena;
    size_t arena_bytes = 0;
    DeviceBlock kv_mem[4];  // key pages, value pages, and (FP8) their scales
    uint16_t *kpool = nullptr, *vpool = nullptr;  // [layers][P, Hkv, page, D]
    size_t layer_pool_elems = 0, kv_bytes = 0;
    // FP8 pages (tl_engine_create_kv, kv8.h): the pools hold one byte per element and the rows' scales live beside them
    int kv_format = TL_KV_BF16;
    float *kscale_pool = nullptr, *vscale_pool = nullptr;  // [layers][P, Hkv, page]
    size_t layer_scale_elems = 0;
    size_t kv_elem_bytes() const { return kv_format == TL_KV_FP8_E4M3 ? 1 : 2; }
    float *layer_ks(int l) const { return kscale_pool ? kscale_pool + (size_t)l * layer_scale_elems : nullptr; }
    float *layer_vs(int l) const { return vscale_pool ? vscale_pool + (size_t)l * layer_scale_elems : nullptr; }
    // what the projection router reads (decode_linear.h): weight copies, matmul workspace, routing options; stream, eps and xn as below
    LinearCtx lin;
    std::vector<TiledW4Mem> tiled_mem;  // the owners of lin.tiled, lin.bf16w and lin.splitk_ws
    std::vector<DeviceBlock> bf16w_mem;
    DeviceBlock splitk_mem;
    size_t tiled_bytes = 0, bf16w_bytes = 0;

    int32_t *block_table = nullptr, *context_lens = nullptr, *tokens = nullptr, *live = nullptr, *produced = nullptr,
            *ring = nullptr, *scratch_ctx = nullptr, *prefill_tokens = nullptr;
    // the shared hand-over buffers (engine_layout.h Act; x_out is the residual stream x): every prefill pass, and the decode steps that
    // do not run on the per-layer buffers below
    Act shared;
    uint16_t *q_t = nullptr, *attn_t = nullptr, *logits = nullptr;
    AttnCtx attn;  // what the decode attention reads (decode_attention.h): geometry, knobs, the slot state it walks, the arena's partials
    // lm_head GEMV of a 1-4-row decode step: per 16-logit tile (max, lowest index) pairs for step_end_kernel (qmv3.h tile_max);
    // tl_engine_set_option "lmhead_tile_max" = 0: step_end reads the logits row again
    f32x2 *lm_tile_max = nullptr;            // [VERIFY_MAX_LEN][vocab / 16]
    bool lm_tile_max_on = true;
    int32_t *verify_ids = nullptr;  // greedy ids of the rows of the last tl_engine_verify
    // tl_engine_verify_sampled: the per-row arrays of its one tl_spec_sample_rows launch (VERIFY_MAX_LEN rows), allocated by the first call
    struct SpecRecord {
        int32_t proposal[VERIFY_MAX_LEN];
        float t_temperature[VERIFY_MAX_LEN];
        int32_t t_top_k[VERIFY_MAX_LEN];
        float t_top_p[VERIFY_MAX_LEN], d_temperature[VERIFY_MAX_LEN];
        int32_t d_top_k[VERIFY_MAX_LEN];
        float d_top_p[VERIFY_MAX_LEN];
        int32_t position[VERIFY_MAX_LEN];
        uint64_t seed[VERIFY_MAX_LEN];
        int32_t accept[VERIFY_MAX_LEN], alt[VERIFY_MAX_LEN];  // (results: behind everything the host writes)
    };
    DeviceBlock spec_mem;
    SpecRecord *spec_rec = nullptr;
    int rows_cap = 0;
    int ring_cap = 4096;

    // the host mirror of block_table / context_lens / live: the page pool, the host arena's records and what each slot holds of them
    // (slot_table.h).  Its calls report edits; apply_edits puts them on the stream.  `step_edits`: the decode step's list, reused
    SlotTable table;
    SlotEdits step_edits;
    DeviceBlock kv_pools_mem;
    tl_kv_pool_desc *kv_pools_dev = nullptr;  // [kv_pools_n] every K / V (and scale) pool, for the tail copy of a hit (kv_copy.h)
    int kv_pools_n = 0;
    std::vector<tl_kv_pool_desc> kv_pools_host;  // the same table on the host (record offsets of kv_swap.h)
    // KV swap (tl_engine_swap_space / _park / _unpark; kv_swap.h, slot_table.h): nothing is allocated before the first swap_space.  A
    // parked slot stays live on the host (the table's slot and every per-slot setting keep their values) and is a slot without a
    // sequence on the device (live 0, context 0, block-table row -1): slot_runs() is what a decode step asks
    DeviceBlock swap_host, swap_staging;  // pinned arena [records][record_bytes]; device staging [swap_staging_pages][record_bytes]
    DeviceBlock swap_offsets_mem;
    size_t *swap_offsets_dev = nullptr;                  // [kv_pools_n] where each pool's bytes start inside a record
    size_t swap_record_bytes = 0;
    int swap_staging_pages = 0;
    long swap_parks = 0, swap_unparks = 0, swap_pages_out = 0, swap_pages_in = 0;
    bool slot_runs(int slot) const { return table.runs(slot); }
    tl_engine_stats stats{};
    // the per-slot settings (slot_settings.h): the host mirrors of sampling, log-probability records, penalties / bias / grammar,
    // truncation, the adapter id and the stop conditions, and the layout of each feature's device block.  Its calls report edits;
    // settings_apply puts them on the stream.  The blocks are allocated by the first call that needs them (settings_blocks; the
    // sampling block with the engine, the adapter ids inside lora_mem); the launches take their addresses from sdev()
    SlotSettings settings;
    DeviceBlock settings_mem[SB_COUNT];
    template <class T>
    T *sdev(int block, size_t off) const {
        return block == SB_LORA ? (T *)((char *)lora_slot_dev + off) : settings_mem[block].at<T>(off);
    }
    const tl_grammar *grammar_of(int slot) const { return (const tl_grammar *)settings.slots[slot].pen.grammar.id; }
    // tl_engine_score: the logits of one block of rows and the per-row targets / results, allocated on first use
    DeviceBlock score_mem;
    uint16_t *score_logits = nullptr;
    int32_t *score_ids = nullptr, *score_argmax = nullptr;
    float *score_lp = nullptr;
    // embeddings (tl_engine_embed / _embed_packed, pool.h): the vectors of a call's finishing sequences [16, hidden] fp32, allocated by the
    // first embed call; the running sums of mean pooling [max_batch, hidden] fp32, allocated by the first MEAN call (how many rows a
    // slot's running sum holds: settings.slots[slot].emb_rows)
    DeviceBlock emb_out_mem, emb_sums_mem;
    float *emb_out = nullptr, *emb_sums = nullptr;
    // LoRA adapters (tl_engine_lora_load / tl_engine_set_lora, lora.h; per slot the adapter id: settings.slots[slot].lora, -1: none):
    // allocated by the first load -- the device table [TL_MAX_LORA_ADAPTERS][layers][4 groups], the per-slot ids the
    // decode step's tiles look up, the tile lists (decode: fixed blocks of 16 rows; prefill: written per pass), the shrink's partials and
    // sums of squares, and the rows of residual + delta ahead of a base projection's residual epilogue
    enum { LORA_QKV, LORA_O, LORA_GU, LORA_DOWN, LORA_GROUPS };
    struct LoraResident {
        DeviceBlock mem;  // the fused matrices of every layer
        size_t bytes = 0;
        int rank = 0;
        std::vector<char> has;  // [layers][groups]: the adapter adapts that group
    };
    std::vector<LoraResident> lora_ad;
    DeviceBlock lora_mem;
    LoraDesc *lora_table = nullptr;
    int32_t *lora_slot_dev = nullptr;
    LoraTile *lora_tiles_decode = nullptr, *lora_tiles_prefill = nullptr;
    float *lora_partial = nullptr, *lora_ss = nullptr;
    uint16_t *lora_tmp = nullptr;
    long lora_steps = 0, lora_prefill_rows = 0;
    bool lora_slot(int slot) const { return settings.slots[slot].lora >= 0; }
    // stop conditions (tl_engine_set_stop, stop.h): a stop launch was enqueued since the records were last read (stop_reconcile)
    bool stop_dirty = false;

    bool warmed = false;
    // a captured decode step: the executable graph and, where the step may ride the AQL route (below), the same nodes as a program of
    // dispatch packets.  Move-only; a plan that goes destroys its graph.  Keyed and kept by replay_route.h
    struct DecodePlan {
        struct ExecDestroy {
            void operator()(hipGraphExec_t exec) const { (void)hipGraphExecDestroy(exec); }
        };
        std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, ExecDestroy> exec;
        std::unique_ptr<AqlProgram> program;
    };
    PlanCache<DecodePlan> plans;
    // AQL replay (aql.h; TL_AQL=1 at create): a captured step also becomes a program of hand-written dispatch packets on the engine's own
    // HSA queue; a plan without a program (a kernel outside the device-only code objects, a node that is not a kernel) stays on hipGraphLaunch
    bool aql_on = false;
    int device = 0;                  // the HIP device the engine was created on: its buffers, its stream, its AQL runtime
    AqlRuntime *aql_rt = nullptr;    // the runtime of that device (aql.h: one per device, process-wide)
    std::unique_ptr<AqlQueue> aql_queue;
    AqlFences aql_fences;
    std::string aql_why;  // why the route is not available to this engine (aql_on false)
    // Per-layer decode activations (common.h, "activations between the launches of a decode step"): with the AQL route every value a launch
    // hands to a later launch of the SAME step lives at an address written once per step -- layer l's x / h / weighted h / qkv / attention
    // rows and partials / SwiGLU rows / sums of squares have their own buffers (1-4 rows: the fused-GEMV route; 36 x ~0.3 MB at Qwen3-4B)
    std::vector<Act> layer_act;  // (5 .. 64 rows, round 5: xw is x_out weighted for the NEXT RMSNorm, planes the slice planes of wo / w_down)
    DeviceBlock layer_act_mem;
    int layer_act_rows = 0;       // rows the per-layer buffers hold (0: none)
    size_t layer_ws_bytes = 0;    // attention partials per layer
    size_t layer_plane_bytes[2] = {0, 0};  // slice planes per layer: [0] wo, [1] w_down
    bool step_written_once = false;  // the last enqueued step used the per-layer buffers throughout (enqueue_step)
    size_t arena_act_off = 0;        // where the activations start inside the arena (behind the state words)
    size_t layer_act_bytes = 0;      // size of layer_act_mem
    // Qwen3-MoE layers (tl_engine_set_moe_layer): router + stacked experts instead of the dense gate|up / w_down of that layer
    std::vector<tl_moe_weights> moe;  // per layer; num_experts == 0: dense
    int moe_k_max = 0, moe_e_max = 0, moe_i_max = 0;
    DeviceBlock moe_ws;  // one allocation: router logits, ids, scores, gate / up / act rows, expert outputs
    size_t moe_ws_bytes = 0;
    uint16_t *moe_logits = nullptr, *moe_scores = nullptr, *moe_gate = nullptr, *moe_up = nullptr, *moe_act = nullptr, *moe_y = nullptr;
    int32_t *moe_ids = nullptr;
    bool is_moe(int l) const { return l < (int)moe.size() && moe[l].num_experts > 0; }
    DeviceBlock rope_table_mem, rope_cur_mem;
    float2 *rope_table = nullptr, *rope_cur = nullptr;
    int rope_positions = 0;
    int logits_rows = 0;
    int logits_slot = -1;  // whose rows the most recent logits are: -1: row i is slot i (a decode step); >= 0: that slot's (a prefill, a verification); -2: a packed prefill's
    // beam search (tl_engine_beam_select, beam.h): the group's scores, the records of one call and the survivors between its two
    // launches, allocated by the first call
    DeviceBlock beam_mem;
    float *beam_scores = nullptr;
    tl_beam_candidate *beam_out = nullptr, *beam_survivors = nullptr;
    // batched verification (tl_engine_verify_batch, verify_attn.h): everything the pass touches besides the weights, the KV pools and
    // the slot state, allocated by the first call -- the activations of 64 rows, their logits, the matmul workspace a 64-row M needs
    // (the engine's own is sized for max(max_batch, max_prefill_rows) rows), the attention partials, the descriptors of one call
    // (uploaded in one copy) and its results
    struct VerifyScratch {
        enum { TOKENS, ROW_SLOT, ROW_POS, SEQ_SLOT, SEQ_ROW0, SEQ_LEN, SEQ_CTX, DESC_ARRAYS };  // the arrays of `desc`, VERIFY_BATCH_ROWS words each
        DeviceBlock mem;
        Act act;           // the hand-over buffers of every layer
        LinearScratch lin;  // what the projection router uses for the duration of a pass: xn (act's), gu, tmp and the matmul workspace
        uint16_t *q = nullptr, *logits = nullptr;
        size_t attn_ws_rows = 0;
        int32_t *desc = nullptr, *greedy = nullptr;
        tl_verify_result *results = nullptr;
        const int32_t *arr(int which) const { return desc + which * VERIFY_BATCH_ROWS; }
        int rows = 0;  // rows of `logits` the last pass wrote (tl_engine_copy_verify_logits)
        // tl_engine_verify_batch_sampled: accept / alt of the pass's rows, allocated by its first call
        DeviceBlock sampled_mem;
        int32_t *accept = nullptr, *alt = nullptr;
    } vb;

    int qkv_dim() const { return (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim; }
    int q_dim() const { return cfg.num_heads * cfg.head_dim; }
    const tl_w4 &head() const { return lm_head.weight_dev ? lm_head : embed; }
    uint16_t *layer_k(int l) const { return (uint16_t *)((char *)kpool + (size_t)l * layer_pool_elems * kv_elem_bytes()); }
    uint16_t *layer_v(int l) const { return (uint16_t *)((char *)vpool + (size_t)l * layer_pool_elems * kv_elem_bytes()); }
};

static int aql_drain(tl_engine *e);
static std::string library_dir();

namespace tl {

// ---- small launch helpers ----------------------------------------------------------------------
// words written on the stream between steps, as (address, value): eight per poke launch
using Pokes = std::vector<std::pair<int32_t *, int32_t>>;
static int poke(tl_engine *e, Pokes &items) {
    for (size_t i = 0; i < items.size(); i += 8) {
        PokeArgs a{};
        a.n = (int)std::min<size_t>(8, items.size() - i);
        for (int j = 0; j < a.n; ++j) {
            a.addr[j] = items[i + j].first;
            a.value[j] = items[i + j].second;
        }
        hipLaunchKernelGGL(poke_kernel, dim3(1), dim3(64), 0, e->stream, a);
    }
    items.clear();
    TL_CHECK_LAUNCH("engine poke");
    return TL_OK;
}
// a float as its word; a 64-bit value (a pointer, a seed) as its two words
static void poke_float(Pokes &pk, float *at, float v) { pk.emplace_back((int32_t *)at, __builtin_bit_cast(int32_t, v)); }
static void poke_u64(Pokes &pk, void *at, uint64_t v) {
    pk.emplace_back((int32_t *)at, (int32_t)(uint32_t)v);
    pk.emplace_back((int32_t *)at + 1, (int32_t)(uint32_t)(v >> 32));
}

// ---- per-slot sampling (sample.h) and log-probabilities (logprob.h) over caller rows; the step-end kernels are in step_end.h ----
// tl_logprob_rows / tl_engine_score: the routine over rows of logits.  grid = rows, block = 1024.
struct LogprobRowsArgs {
    const uint16_t *logits;  // [rows, vocab]
    int vocab, top_n;
    const int32_t *ids;      // [rows] the token whose log-probability is asked for (< 0: NaN); nullptr: each row's greedy id
    float *logprob;          // [rows]
    int32_t *top_ids;        // [rows, top_n] (top_n > 0)
    float *top_logprobs;     // [rows, top_n]
    int32_t *argmax;         // [rows] greedy ids, or nullptr
};

static __global__ __launch_bounds__(1024) void logprob_rows_kernel(const LogprobRowsArgs a) {
    __shared__ SampleSmem sm;
    __shared__ LogprobSmem ls;
    const int i = blockIdx.x;
    const SmpRow row(a.logits + (long)i * a.vocab, a.vocab);
    const float lse = lp_row(row, __builtin_nanf(""), a.top_n, sm, ls);
    if (threadIdx.x == 0) {
        const int t = a.ids ? a.ids[i] : ls.greedy;
        a.logprob[i] = t >= 0 && t < a.vocab ? BF16::to_float(row.lg[t]) - lse : __builtin_nanf("");
        if (a.argmax) a.argmax[i] = ls.greedy;
    }
    if ((int)threadIdx.x < a.top_n) {
        a.top_ids[(long)i * a.top_n + threadIdx.x] = (int32_t)ls.rec[1 + threadIdx.x];
        a.top_logprobs[(long)i * a.top_n + threadIdx.x] = __uint_as_float(ls.rec[1 + LP_MAX_TOP + threadIdx.x]);
    }
}

// tl_sample_logits: the same selection over caller rows, parameters per row.  grid = rows, block = 1024.
static __global__ __launch_bounds__(1024) void sample_rows_kernel(const uint16_t *logits, int vocab, const float *temperature, const int32_t *top_k,
                                                                  const float *top_p, const uint64_t *seed, const int32_t *position, int32_t *ids) {
    __shared__ SampleSmem sm;
    const int i = blockIdx.x;
    const SmpRow row(logits + (long)i * vocab, vocab);
    const int tok = smp_select(row, __builtin_nanf(""), temperature[i], top_k[i], top_p[i], seed[i], (uint32_t)position[i], sm);
    if (threadIdx.x == 0) ids[i] = tok;
}

// StepEndArgs over the engine's state: rows of `logits` for slots slot0.., the context advance (1: decode; 0: a prefill sets it on the host
// side) and the next embedding rows into x; tile maxima, sums of squares and stamps where the step has them
static StepEndArgs step_end_args(const tl_engine *e, const uint16_t *logits, int slot0, int advance, uint16_t *x, const f32x2 *tile_max = nullptr,
                                 int tiles = 0, float *ss_out = nullptr, prof_t *prof = nullptr) {
    const tl_engine_config &c = e->cfg;
    StepEndArgs s{};
    s.logits = logits;
    s.vocab = c.vocab_size;
    s.slot0 = slot0;
    s.tokens = e->tokens;
    s.context_lens = e->context_lens;
    s.live = e->live;
    s.produced = e->produced;
    s.ring = e->ring;
    s.ring_cap = e->ring_cap;
    s.advance = advance;
    s.emb_w = e->embed.weight_dev;
    s.emb_s = (const uint16_t *)e->embed.scales_dev;
    s.emb_b = (const uint16_t *)e->embed.biases_dev;
    s.x = x;
    s.hidden = c.hidden_size;
    s.rope_table = e->rope_table;
    s.rope_cur = e->rope_cur;
    s.rope_positions = e->rope_positions;
    s.rope_half = c.head_dim / 2;
    s.ss_out = ss_out;
    s.prof = prof;
    s.tile_max = tile_max;
    s.tiles = tiles;
    return s;
}

// step end of a decode step / a prefill's last row: greedy kernel, its sampling twin when the plan samples, or the logprob twin
// (which also samples) when a slot records log-probabilities
// `raw`: the rows of the model's logits where s.logits are processed rows (logit_process.h) -- the logprob twin records from them
static void launch_step_end(tl_engine *e, const StepEndArgs &s, int rows, bool samples, bool logprobs, const uint16_t *raw = nullptr) {
    const SlotSettings::Offsets &at = e->settings.at;
    const SampleStepEndArgs q{s, e->sdev<float>(SB_SAMPLE, at.smp_temp), e->sdev<int32_t>(SB_SAMPLE, at.smp_topk), e->sdev<float>(SB_SAMPLE, at.smp_topp),
                              e->sdev<uint64_t>(SB_SAMPLE, at.smp_seed)};
    if (logprobs) {
        LogprobStepEndArgs l{q, e->sdev<int32_t>(SB_LOGPROB, at.lp_topn), e->sdev<uint32_t>(SB_LOGPROB, at.lp_ring), e->sdev<uint32_t>(SB_LOGPROB, at.lp_pending), nullptr};
        if (raw) l.choice = s.logits, l.q.s.logits = raw;
        hipLaunchKernelGGL(logprob_step_end_kernel, dim3(rows), dim3(1024), 0, e->stream, l);
    } else if (samples) {
        hipLaunchKernelGGL(sample_step_end_kernel, dim3(rows), dim3(1024), 0, e->stream, q);
    } else {
        hipLaunchKernelGGL(step_end_kernel, dim3(rows), dim3(1024), 0, e->stream, s);
    }
}

// tl_engine_score: rows of the lm_head per W4 GEMM + logprob launch (the scratch holds one block of logits: 311 MB at Qwen3's vocabulary)
constexpr int SCORE_BLOCK_ROWS = 1024;

// ---- the per-slot settings on the device (slot_settings.h) ----------------------------------------------------------------------------
// the sizes the record's layouts are made of are the device headers'
static_assert(sizeof(StopMirror) == sizeof(StopRecord) && offsetof(StopMirror, reason) == offsetof(StopRecord, reason) &&
                  offsetof(StopMirror, context) == offsetof(StopRecord, context) && offsetof(StopMirror, cut_bytes) == offsetof(StopRecord, cut_bytes),
              "StopMirror is the device's stop record");
static_assert(offsetof(GrammarRecord, tag) == 0 && offsetof(GrammarRecord, state) == 4 && offsetof(GrammarStackRecord, rec) == 0,
              "a grammar record starts with {tag, state}; a stack grammar's with the packed word whose low half is the tag");
static_assert(sizeof(GrammarDev *) == 8 && sizeof(StopDev *) == 8 && LPR_MAX_BIAS == TL_MAX_LOGIT_BIAS, "pointers are two words");
static SlotSettings::Sizes settings_sizes(const tl_engine *e) {
    return {e->cfg.max_batch, e->cfg.vocab_size, e->ring_cap, LP_RECORD_WORDS, LP_MAX_TOP, LPR_MAX_BIAS, (int)sizeof(GrammarRecord), (int)sizeof(GrammarStackRecord),
            (int)sizeof(StopRecord), SMP_MAX_VOCAB, LORA_NONE, e->cfg.max_pages_per_seq * e->cfg.page_size, DRY_MAX_BREAKERS, DRY_MAX_MATCH, e->cfg.max_pages_per_seq * e->cfg.page_size, LOOKUP_OUT_WORDS};
}

// What the allocation of each block reports when it fails (fill: the memsets and the launch that give a fresh block its first values), and
// whether the block counts as workspace
struct SettingsBlockTexts {
    const char *malloc_failed, *fill_failed;
    bool counted;
};
static const SettingsBlockTexts SETTINGS_BLOCK_TEXTS[SB_COUNT] = {
    {"engine_create: hipMalloc(sampling) failed", "engine_create: memset failed", false},
    {"engine_set_logprobs: hipMalloc(records) failed", nullptr, false},  // (the fill's text: below)
    {"engine: hipMalloc(logit processing) failed", "engine: memset(logit processing) failed", true},
    {"engine: hipMalloc(grammar slots) failed", "engine: memset(grammar slots) failed", true},
    {"engine: hipMalloc(stack grammar slots) failed", "engine: memset(stack grammar slots) failed", true},
    {"engine: hipMalloc(truncation) failed", "engine: memset(truncation) failed", true},
    {"engine_set_stop: hipMalloc(stop records) failed", "engine_set_stop: memset(stop records) failed", true},
    {nullptr, nullptr, false},  // (the adapter ids: inside lora_mem, lora_alloc)
    {"engine_set_dry: hipMalloc(sequence rows) failed", "engine_set_dry: memset(sequence rows) failed", true},
    {"engine_set_lookup: hipMalloc(history rows) failed", "engine_set_lookup: memset(history rows) failed", true},
};
// the blocks of `needs` that do not exist yet, each from its layout: all-or-nothing per block, filled on the engine stream
static int settings_blocks(tl_engine *e, unsigned needs) {
    for (int b = 0; b < SB_COUNT; ++b) {
        if (b == SB_LORA || !(needs >> b & 1u) || e->settings_mem[b]) continue;
        const BlockLayout &lay = e->settings.layout(b);
        const SettingsBlockTexts &t = SETTINGS_BLOCK_TEXTS[b];
        TL_TRY(alloc_filled(e->settings_mem[b], lay.bytes, t.malloc_failed, [&](char *m) -> int {
            for (const BlockFill &f : lay.fill) {
                if (f.word == 0u || f.word == 0xffffffffu) {
                    const hipError_t he = hipMemsetAsync(m + f.off, (int)(f.word & 0xffu), f.bytes, e->stream);
                    if (he == hipSuccess) continue;
                    // (the log-probability records': the text TL_HIP gave this call when it stood on e->lp_mem)
                    return fail(TL_ERR_HIP, t.fill_failed ? std::string(t.fill_failed)
                                                          : std::string("hipMemsetAsync(e->lp_mem, 0xff, (size_t)B * 4 + (size_t)B * rec, e->stream): ") + hipGetErrorString(he));
                }
                const int n = (int)(f.bytes / 4);
                hipLaunchKernelGGL(fill_i32_kernel, dim3(ceil_div((long)n, 256)), dim3(256), 0, e->stream, (int32_t *)(m + f.off), (int32_t)f.word, n);
                TL_CHECK_LAUNCH("engine logit-processing init");
            }
            return TL_OK;
        }));
        if (t.counted) e->stats.workspace_bytes += lay.bytes;
        e->settings.created(b);
    }
    return TL_OK;
}
// An edit list in order on the engine stream.  Words join `pk` -- the caller's own words may wait there -- and are poked, eight per
// launch, ahead of the next copy, fill or upload and at the end; within one list no word is written twice
static int settings_apply(tl_engine *e, const SettingsEdits &ed, Pokes &pk) {
    for (const SettingsEdit &x : ed.list) {
        char *at = e->sdev<char>(x.block, x.off);
        if (x.kind == SettingsEdit::WORD) {
            pk.emplace_back((int32_t *)at, x.word);
            continue;
        }
        if (!pk.empty()) TL_TRY(poke(e, pk));
        if (x.kind == SettingsEdit::COPY) TL_HIP(hipMemcpyAsync(at, e->sdev<char>(x.block, x.from), x.bytes, hipMemcpyDeviceToDevice, e->stream));
        else if (x.kind == SettingsEdit::FILL) TL_HIP(hipMemsetAsync(at, 0, x.bytes, e->stream));
        else TL_HIP(hipMemcpyAsync(at, x.host, x.bytes, hipMemcpyHostToDevice, e->stream));
    }
    return pk.empty() ? TL_OK : poke(e, pk);
}
// A setter's call of the record: the refusal, or the blocks it needs and its edits.  A block that cannot be made leaves the slot's
// mirror as it was
template <class Call>
static int settings_set(tl_engine *e, int slot, Pokes &pk, Call call) {
    SettingsEdits ed;
    SlotSettings::State before = e->settings.slots[slot];
    if (const char *why = call(ed)) return fail(TL_ERR_INVALID, why);
    const int rc = settings_blocks(e, ed.needs);
    if (rc != TL_OK) {
        e->settings.slots[slot] = std::move(before);
        return rc;
    }
    return settings_apply(e, ed, pk);
}

// the processing launch over `rows` rows of raw logits for slots slot0 .. (logit_process.h): processed rows into `out`.  A decode step
// passes the pending tokens (counted before the row is processed); a prefill's last row has none to count.
static void launch_logit_process(tl_engine *e, const uint16_t *logits, uint16_t *out, int rows, int slot0, const int32_t *tokens, bool grammar,
                                 bool stack, ProfCtx *pc) {
    const SlotSettings::Offsets &at = e->settings.at;
    const LogitProcessArgs a{logits, out, e->cfg.vocab_size, slot0, e->sdev<uint16_t>(SB_PROCESS, at.pen_history), e->sdev<float>(SB_PROCESS, at.pen_rep),
                             e->sdev<float>(SB_PROCESS, at.pen_pres), e->sdev<float>(SB_PROCESS, at.pen_freq), e->sdev<int32_t>(SB_PROCESS, at.pen_bias_n),
                             e->sdev<int32_t>(SB_PROCESS, at.pen_bias_ids), e->sdev<float>(SB_PROCESS, at.pen_bias_values), tokens, pc ? pc->buf : nullptr,
                             grammar ? e->sdev<const GrammarDev *>(SB_GRAMMAR, at.gr_ptr) : nullptr,
                             grammar ? e->sdev<GrammarRecord>(SB_GRAMMAR, at.gr_state) : nullptr, grammar ? e->context_lens : nullptr,
                             tokens ? e->live : nullptr};
    const dim3 grid(ceil_div(e->cfg.vocab_size, LPR_CHUNK), rows);
    if (stack) hipLaunchKernelGGL(logit_process_stack_kernel, grid, dim3(LPR_THREADS), 0, e->stream, LogitProcessStackArgs{a, e->sdev<GrammarStackRecord>(SB_STACK, 0)});
    else if (grammar) hipLaunchKernelGGL(logit_process_kernel<true>, grid, dim3(LPR_THREADS), 0, e->stream, a);
    else hipLaunchKernelGGL(logit_process_kernel<false>, grid, dim3(LPR_THREADS), 0, e->stream, a);
    if (pc) prof_after(pc, 7, (int)(grid.x * grid.y));
}

// the two launches of DRY and the n-gram ban (dry.h) over `rows` processed rows for slots slot0 .., rewritten in place.  A decode step
// passes the fed tokens, which the match launch stores at S[e] = S[context length]; a prefill's row has recorded its ids already and
// ends at context length - 1
static DryArgs dry_args(tl_engine *e, uint16_t *rows, int slot0, const int32_t *tokens, prof_t *prof) {
    const SlotSettings::Offsets &at = e->settings.at;
    DryArgs a{};
    a.seq = e->sdev<int32_t>(SB_DRY, at.dry_seq), a.table = e->sdev<uint32_t>(SB_DRY, at.dry_table), a.rows = rows;
    a.cap = e->settings.sz.dry_seq_cap, a.vocab = e->cfg.vocab_size, a.slot0 = slot0, a.pos_bias = tokens ? 0 : -1;
    a.pos = e->context_lens, a.tokens = tokens, a.live = e->live;
    a.multiplier = e->sdev<float>(SB_DRY, at.dry_mult), a.base = e->sdev<float>(SB_DRY, at.dry_base);
    a.allowed = e->sdev<int32_t>(SB_DRY, at.dry_allowed), a.range = e->sdev<int32_t>(SB_DRY, at.dry_range);
    a.ngram = e->sdev<int32_t>(SB_DRY, at.dry_ngram), a.start = e->sdev<int32_t>(SB_DRY, at.dry_s0);
    a.n_breakers = e->sdev<int32_t>(SB_DRY, at.dry_nbreak), a.breakers = e->sdev<int32_t>(SB_DRY, at.dry_breakers);
    a.prof = prof;
    return a;
}
static void launch_dry(tl_engine *e, uint16_t *processed, int rows, int slot0, const int32_t *tokens, ProfCtx *pc) {
    const DryArgs a = dry_args(e, processed, slot0, tokens, pc ? pc->buf : nullptr);
    hipLaunchKernelGGL(dry_match_kernel, dim3(rows), dim3(DRY_MATCH_THREADS), 0, e->stream, a);
    if (pc) prof_after(pc, 7, rows);
    const dim3 grid(ceil_div(e->cfg.vocab_size, DRY_APPLY_CHUNK), rows);
    hipLaunchKernelGGL(dry_apply_kernel, grid, dim3(DRY_APPLY_THREADS), 0, e->stream, a);
    if (pc) prof_after(pc, 7, (int)(grid.x * grid.y));
}
// a chunk's uploaded ids (at `tokens_dev`) enter the sequence row of a slot that records them, at positions start ..
static void launch_dry_record(tl_engine *e, int slot, const int32_t *tokens_dev, int n, int start) {
    const int cap = e->settings.sz.dry_seq_cap;
    const DryRecordArgs a{tokens_dev, e->sdev<int32_t>(SB_DRY, e->settings.at.dry_seq) + (size_t)slot * cap, n, start, cap};
    hipLaunchKernelGGL(dry_record_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, e->stream, a);
}

// ---- prompt lookup (lookup.h): the history row H of an armed slot; the accounting is the settings record's (slot_settings.h) ----
static int32_t *lookup_row_dev(tl_engine *e, int slot) {
    return e->sdev<int32_t>(SB_LOOKUP, e->settings.at.lk_seq) + (size_t)slot * e->settings.sz.lookup_seq_cap;
}
// ids at `tokens_dev` (uploaded, or the slot's pending token) enter H at positions start ..
static int lookup_record(tl_engine *e, int slot, const int32_t *tokens_dev, int n, int start) {
    const LookupRecordArgs a{tokens_dev, lookup_row_dev(e, slot), n, start, e->settings.sz.lookup_seq_cap};
    hipLaunchKernelGGL(lookup_record_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, e->stream, a);
    TL_CHECK_LAUNCH("engine lookup recording");
    return TL_OK;
}
// H of an armed slot reaches the slot's context: the ids of the decode steps since the last recording come out of the token ring (the
// steps themselves record nothing).  No launch where the slot is not armed or not behind
static int lookup_catch_up(tl_engine *e, int slot) {
    const Slot &t = e->table.slots[slot];
    if (!e->settings.lookup_behind(slot, t.ctx)) return TL_OK;
    TL_TRY(aql_drain(e));  // (steps of the AQL route wrote the ring)
    const int rec = e->settings.slots[slot].lk_rec;
    const LookupCatchUpArgs a{lookup_row_dev(e, slot), e->ring + (size_t)slot * e->ring_cap, e->ring_cap, rec, t.ctx, t.produced, e->settings.sz.lookup_seq_cap};
    hipLaunchKernelGGL(lookup_catch_up_kernel, dim3(std::min(ceil_div(t.ctx - rec, 256), 64)), dim3(256), 0, e->stream, a);
    TL_CHECK_LAUNCH("engine lookup catch-up");
    e->settings.lookup_caught_up(slot, t.ctx);
    return TL_OK;
}
// the pending token of an armed slot -- one the ring does not hold: tl_engine_set_token's, a fork's or move's, the one the slot was
// armed with -- is stored at H[ctx], behind whatever put it into tokens[slot]
static int lookup_store_pending(tl_engine *e, int slot) {
    if (!e->settings.lookup_on(slot)) return TL_OK;
    TL_TRY(lookup_catch_up(e, slot));
    TL_TRY(lookup_record(e, slot, e->tokens + slot, 1, e->table.slots[slot].ctx));
    e->settings.lookup_pending(slot, e->table.slots[slot].ctx);
    return TL_OK;
}
// a chunk of n uploaded ids at `tokens_dev` is appended to the slot at position `start` (its context length)
static int lookup_record_chunk(tl_engine *e, int slot, const int32_t *tokens_dev, int n, int start) {
    if (!e->settings.lookup_on(slot)) return TL_OK;
    TL_TRY(lookup_catch_up(e, slot));
    TL_TRY(lookup_record(e, slot, tokens_dev, n, start));
    e->settings.lookup_recorded(slot, start, n);
    return TL_OK;
}
// ahead of `steps` decode steps over slots [0, batch): a slot whose unrecorded ids would outrun the ring is caught up first; `restart`
// takes the slots a single call outruns the ring for (lookup_steps_done starts their history over behind the call)
static int lookup_before_steps(tl_engine *e, int batch, long steps, std::vector<int> *restart) {
    for (int b = 0; b < batch; ++b) {
        if (!e->slot_runs(b) || !e->settings.lookup_on(b)) continue;
        if (e->settings.lookup_pending_unknown(b, e->table.slots[b].ctx)) TL_TRY(lookup_store_pending(e, b));
        const SlotSettings::LookupDecode d = e->settings.lookup_before_decode(b, e->table.slots[b].ctx, steps);
        if (d == SlotSettings::LOOKUP_CATCH_UP) TL_TRY(lookup_catch_up(e, b));
        if (d == SlotSettings::LOOKUP_RESTART && restart) restart->push_back(b);
    }
    return TL_OK;
}
static void lookup_steps_done(tl_engine *e, const std::vector<int> &restart) {
    for (int b : restart) e->settings.lookup_restart(b, e->table.slots[b].ctx);
}

// the truncation launch over `rows` rows for slots slot0 .. (the rows the choice would be made from -> filtered rows into `out`), and the
// Mirostat update launch behind the step end; `row0`: the index of the first row inside the engine's row buffers
static void launch_truncate(tl_engine *e, const uint16_t *rows_in, uint16_t *out, int rows, int slot0, int row0, ProfCtx *pc) {
    const SlotSettings::Offsets &at = e->settings.at;
    const TruncateArgs a{rows_in, out, e->cfg.vocab_size, slot0, e->sdev<float>(SB_SAMPLE, at.smp_temp), e->sdev<float>(SB_TRUNC, at.trn_minp),
                         e->sdev<float>(SB_TRUNC, at.trn_typ), e->sdev<float>(SB_TRUNC, at.trn_mu), e->sdev<float>(SB_TRUNC, at.trn_logsum) + row0,
                         pc ? pc->buf : nullptr};
    hipLaunchKernelGGL(truncate_rows_kernel, dim3(rows), dim3(1024), 0, e->stream, a);
    if (pc) prof_after(pc, 7, rows);
}
static void launch_mirostat_update(tl_engine *e, const uint16_t *filtered, int rows, int slot0, int row0, ProfCtx *pc) {
    const SlotSettings::Offsets &at = e->settings.at;
    const MirostatUpdateArgs a{filtered, e->cfg.vocab_size, slot0, e->tokens, e->sdev<float>(SB_SAMPLE, at.smp_temp), e->sdev<float>(SB_TRUNC, at.trn_logsum) + row0,
                               e->sdev<float>(SB_TRUNC, at.trn_tau), e->sdev<float>(SB_TRUNC, at.trn_eta), e->sdev<float>(SB_TRUNC, at.trn_mu), e->live,
                               pc ? pc->buf : nullptr};
    hipLaunchKernelGGL(mirostat_update_kernel, dim3(rows), dim3(64), 0, e->stream, a);
    if (pc) prof_after(pc, 7, rows);
}

// ---- LoRA adapters (lora.h) ---------------------------------------------------------------------------
// input and output columns of a projection group and how its output columns map to segments
struct LoraShape {
    int in, out, seg_mode, seg_end0, seg_end1;
};
static LoraShape lora_shape(const tl_engine *e, int group) {
    const tl_engine_config &c = e->cfg;
    const int q_dim = e->q_dim(), kv_dim = c.num_kv_heads * c.head_dim;
    switch (group) {
        case tl_engine::LORA_QKV: return {c.hidden_size, e->qkv_dim(), LORA_SEG_BLOCKS, q_dim, q_dim + kv_dim};
        case tl_engine::LORA_O: return {q_dim, c.hidden_size, LORA_SEG_PLAIN, 0, 0};
        case tl_engine::LORA_GU: return {c.hidden_size, 2 * c.intermediate_size, LORA_SEG_INTERLEAVED, 0, 0};
        default: return {c.intermediate_size, c.hidden_size, LORA_SEG_PLAIN, 0, 0};
    }
}
static int lora_tiles_cap(const tl_engine *e) { return std::max(lora_max_tiles(e->rows_cap, PACKED_MAX_SEQS), ceil_div(e->cfg.max_batch, LORA_TILE)); }
// the first load: the device table (all zero: nothing adapted), the per-slot ids (all none), the tile lists and the workspaces
static int lora_alloc(tl_engine *e) {
    if (e->lora_mem) return TL_OK;
    const tl_engine_config &c = e->cfg;
    const int in_max = std::max(std::max(c.hidden_size, e->q_dim()), c.intermediate_size);
    const int cap = lora_tiles_cap(e), decode_tiles = ceil_div(c.max_batch, LORA_TILE);
    Carve carve;
    const size_t table_bytes = (size_t)TL_MAX_LORA_ADAPTERS * c.num_layers * tl_engine::LORA_GROUPS * sizeof(LoraDesc);
    const size_t o_table = carve(table_bytes), o_slot = carve(e->settings.layout(SB_LORA).bytes);
    const size_t o_td = carve((size_t)decode_tiles * sizeof(LoraTile)), o_tp = carve((size_t)cap * sizeof(LoraTile));
    const size_t o_part = carve(lora_partial_floats(cap, in_max) * 4), o_ss = carve(lora_ss_floats(cap, in_max) * 4);
    const size_t o_tmp = carve((size_t)e->rows_cap * c.hidden_size * 2);
    std::vector<LoraTile> tiles;
    lora_lookup_tiles(c.max_batch, tiles);
    TL_TRY(alloc_filled(e->lora_mem, carve.off, "engine_lora_load: hipMalloc(adapter table and workspaces) failed", [&](char *m) -> int {
        hipError_t rc = hipMemset(m + o_table, 0, table_bytes);
        if (rc == hipSuccess) rc = hipMemset(m + o_slot, 0xff, e->settings.layout(SB_LORA).bytes);
        if (rc == hipSuccess) rc = hipMemcpy(m + o_td, tiles.data(), tiles.size() * sizeof(LoraTile), hipMemcpyHostToDevice);
        return rc == hipSuccess ? TL_OK : fail(TL_ERR_HIP, std::string("engine_lora_load: ") + hipGetErrorString(rc));
    }));
    char *mem = e->lora_mem.at();
    e->lora_table = (LoraDesc *)(mem + o_table), e->lora_slot_dev = (int32_t *)(mem + o_slot);
    e->lora_tiles_decode = (LoraTile *)(mem + o_td), e->lora_tiles_prefill = (LoraTile *)(mem + o_tp);
    e->lora_partial = (float *)(mem + o_part), e->lora_ss = (float *)(mem + o_ss), e->lora_tmp = (uint16_t *)(mem + o_tmp);
    e->lora_ad.resize(TL_MAX_LORA_ADAPTERS);
    e->settings.created(SB_LORA);
    return TL_OK;
}
// One adapted projection group of layer l over `n_tiles` tiles: the shrink and the expand launch (lora.h).  norm_w: x is the row ahead
// of that RMSNorm (a decode step), else the row the base projection reads
static int lora_group(tl_engine *e, int l, int group, const LoraTile *tiles_dev, int n_tiles, int total_rows, const uint16_t *x, const void *norm_w,
                      int mode, const uint16_t *base, uint16_t *dst) {
    const LoraShape s = lora_shape(e, group);
    LoraCall c;
    c.table = e->lora_table, c.stride = e->cfg.num_layers * tl_engine::LORA_GROUPS, c.index = l * tl_engine::LORA_GROUPS + group;
    c.n_adapters = TL_MAX_LORA_ADAPTERS, c.row_adapter = e->lora_slot_dev, c.tiles_dev = tiles_dev, c.n_tiles = n_tiles, c.total_rows = total_rows;
    c.x = x, c.in = s.in, c.out = s.out, c.norm_w = (const uint16_t *)norm_w, c.eps = e->cfg.rms_norm_eps;
    c.partial = e->lora_partial, c.ss = e->lora_ss, c.seg_mode = s.seg_mode, c.seg_end0 = s.seg_end0, c.seg_end1 = s.seg_end1;
    c.mode = mode, c.base = base, c.dst = dst;
    return lora_apply(c, e->stream);
}

// ---- stop conditions (stop.h) ---------------------------------------------------------------------------------------
// Host mirrors after a stop.  The mirrors advance per step for every running slot, so a slot that froze in mid-call leaves them ahead of
// the device.  Behind any call that enqueued a stop launch: wait for the stream (and the AQL queue), read the records in one copy, and
// for every slot that newly stopped take the device's context length -- `produced` went up with it, one per step -- and mark the slot
// stopped (slot_table.h).  Pages reserved for steps the slot did not take stay with it, as after tl_engine_reserve.
static int stop_reconcile(tl_engine *e) {
    if (!e->stop_dirty) return TL_OK;
    TL_TRY(aql_drain(e));
    TL_HIP(hipStreamSynchronize(e->stream));
    std::vector<StopMirror> read(e->cfg.max_batch);
    TL_HIP(hipMemcpy(read.data(), e->sdev<StopRecord>(SB_STOP, e->settings.at.stop_rec), read.size() * sizeof(StopRecord), hipMemcpyDeviceToHost));
    e->stop_dirty = false;
    std::vector<SlotSettings::StopEvent> stopped;
    e->settings.stop_records_read(read.data(), [e](int b) -> const Slot & { return e->table.slots[b]; }, stopped);
    for (const SlotSettings::StopEvent &s : stopped) e->table.stop(s.slot, s.context, s.produced);
    return TL_OK;
}

// the stop launch over `rows` rows for slots slot0 .., behind the step end (and the Mirostat update)
static void launch_stop(tl_engine *e, int rows, int slot0, ProfCtx *pc) {
    const SlotSettings::Offsets &at = e->settings.at;
    const StopArgs a{e->tokens, slot0, e->sdev<const StopDev *>(SB_STOP, at.stop_sets), nullptr, e->sdev<int32_t>(SB_STOP, at.stop_armed),
                     e->sdev<int32_t>(SB_STOP, at.stop_max_new), e->sdev<int32_t>(SB_STOP, at.stop_automaton), e->sdev<StopRecord>(SB_STOP, at.stop_rec), e->live,
                     e->context_lens, pc ? pc->buf : nullptr};
    hipLaunchKernelGGL(stop_check_kernel, dim3(rows), dim3(64), 0, e->stream, a);
    if (pc) prof_after(pc, 7, rows);
    e->stop_dirty = true;
}

// ---- which launches a step needs ---------------------------------------------------------------------------------------------------
// (the key bits of a plan and the features that keep it on hipGraphLaunch: replay_route.h)
// the plan of slots [slot0, slot0 + n), re-derived from the slots' parameters by every call that enqueues or replays a step: a decode step
// asks over [0, batch), a prefill's first token over its one slot
static StepFeatures step_features(const tl_engine *e, int slot0, int n) {
    return e->settings.features(slot0, n, [e](int slot) { return e->slot_runs(slot); });
}
// does the slot, taking part in a step, process its logits?
static bool step_processes_slot(const tl_engine *e, int slot) { return e->settings.processes(slot, e->slot_runs(slot)); }
// ... and does it record the ids it is fed (dry.h)?
static bool step_records_slot(const tl_engine *e, int slot) { return e->settings.records(slot, e->slot_runs(slot)); }

// The chain behind the lm_head over `rows` raw rows -- rows [row0, row0 + rows) of the engine's row buffers, slots slot0 .. -- in the one
// order a decode step and a prefill's first token share: processing (logit_process.h), truncation (truncate.h), the step end, the
// Mirostat update, the stop check (stop.h), each where `f` has it.
//   advance, x, ss_out: the step end's context advance, where the next embedding rows go and their sums of squares (step_end_args)
//   tile_max, tiles: the lm_head's per-tile pairs; they describe the raw rows, so only a step that neither processes nor truncates uses them
//   tokens: the pending tokens a decode step's processing launch counts first (e->tokens); a prefill's row has none (null)
static void launch_logit_chain(tl_engine *e, const uint16_t *raw, int row0, int rows, int slot0, int advance, uint16_t *x, const f32x2 *tile_max,
                               int tiles, float *ss_out, const int32_t *tokens, const StepFeatures &f, ProfCtx *pc) {
    const size_t at = (size_t)row0 * e->cfg.vocab_size;
    const uint16_t *choice = raw;  // the rows the token is chosen from
    if (f.processes) {  // raw rows -> processed rows (rows of slots that do not process are copied)
        launch_logit_process(e, choice, e->sdev<uint16_t>(SB_PROCESS, e->settings.at.pen_rows) + at, rows, slot0, tokens, f.grammar, f.stack_grammar, pc);
        choice = e->sdev<uint16_t>(SB_PROCESS, e->settings.at.pen_rows) + at;
        if (f.dry) launch_dry(e, e->sdev<uint16_t>(SB_PROCESS, e->settings.at.pen_rows) + at, rows, slot0, tokens, pc);
    }
    if (f.truncates) {  // ... -> filtered rows (rows of slots that do not truncate are copied)
        launch_truncate(e, choice, e->sdev<uint16_t>(SB_TRUNC, e->settings.at.trn_rows) + at, rows, slot0, row0, pc);
        choice = e->sdev<uint16_t>(SB_TRUNC, e->settings.at.trn_rows) + at;
    }
    const bool maxima = tile_max && choice == raw;
    const StepEndArgs s = step_end_args(e, choice, slot0, advance, x, maxima ? tile_max : nullptr, maxima ? tiles : 0, ss_out, pc ? pc->buf : nullptr);
    launch_step_end(e, s, rows, f.samples, f.logprobs, choice != raw ? raw : nullptr);  // (the logprob twin records from the raw rows)
    if (pc) prof_after(pc, 7, rows);
    if (f.truncates) launch_mirostat_update(e, choice, rows, slot0, row0, pc);
    if (f.stop) launch_stop(e, rows, slot0, pc);
}

// The router's launch over `rows` rows of router logits [rows, E]: ids / scores [rows, top_k] (engine_moe_mlp and tl_moe_route_rows).
static void moe_route_launch(const uint16_t *logits, int rows, int E, int k, int norm, int32_t *ids, uint16_t *scores, hipStream_t st) {
    hipLaunchKernelGGL(moe_route_kernel, dim3(rows), dim3(256), 0, st, logits, E, k, norm, ids, scores);
}

// The expert rows of a MoE MLP: rows x top_k of them, token-major, the token's experts in the order of its ids.  Side by side in one
// block, in this order (tl_moe_experts_rows hands the block to its caller): gate, up, act [rows * k, I], y [rows * k, D].
struct MoeExpertRows {
    uint16_t *gate, *up, *act, *y;
};
inline size_t moe_expert_rows_bytes(int rows, int k, int D, int I) { return (size_t)rows * k * (3 * (size_t)I + D) * 2; }
inline MoeExpertRows moe_expert_rows_at(void *base, int rows, int k, int I) {
    uint16_t *p = (uint16_t *)base;
    const size_t n = (size_t)rows * k * I;
    return {p, p + n, p + 2 * n, p + 3 * n};
}

// Everything of a MoE MLP behind the router, five launches (engine_moe_mlp and tl_moe_experts_rows): gathered gate and up GEMVs (an
// expert per expert row, the activation row of its token), SiLU x up, gathered down GEMV, weighted sum + residual.
static int moe_experts_launch(const tl_moe_weights &m, const uint16_t *xn, const uint16_t *h, const int32_t *ids, const uint16_t *scores,
                              const MoeExpertRows &w, uint16_t *out, int rows, int D, hipStream_t st) {
    const int E = m.num_experts, k = m.experts_per_token, I = m.intermediate_size;
    const int er = rows * k;  // expert rows: token-major, the token's top_k experts in descending probability
    TL_TRY(gather_qmv_bf16(m.gate_scales_dev, m.gate_biases_dev, xn, m.gate_dev, ids, w.gate, er, D, I, E, k, st));
    TL_TRY(gather_qmv_bf16(m.up_scales_dev, m.up_biases_dev, xn, m.up_dev, ids, w.up, er, D, I, E, k, st));
    const long n8 = (long)er * I / 8;
    hipLaunchKernelGGL(moe_silu_mul_kernel, dim3(ceil_div(n8, 256)), dim3(256), 0, st, w.gate, w.up, w.act, n8);
    TL_TRY(gather_qmv_bf16(m.down_scales_dev, m.down_biases_dev, w.act, m.down_dev, ids, w.y, er, I, D, E, 1, st));
    hipLaunchKernelGGL(moe_combine_kernel, dim3(rows), dim3(256), 0, st, w.y, scores, h, out, D, k);
    return TL_OK;
}

// The MLP of a Qwen3-MoE layer over `rows` activation rows: xn = RMSNorm(h) is given; out = h + sum_j score_j * expert_j(xn)
// (reference: moe.py:69-89 inside qwen3_week3.py:204-205).  Every launch reads device-resident ids: graph-capturable.
static int engine_moe_mlp(tl_engine *e, int l, const uint16_t *xn, const uint16_t *h, uint16_t *out, int rows, ProfCtx *pc) {
    const tl_moe_weights &m = e->moe[l];
    const int k = m.experts_per_token;
    TL_REQUIRE(e->moe_ws && rows <= e->rows_cap && (long)rows * k <= 65535, "engine: MoE workspace missing or too many expert rows");
    // router logits [rows, E] through the reference-semantics matmul (quantized_linear of the router, moe.py:44)
    TL_TRY(engine_qmm(e->lin, m.router, xn, e->moe_logits, rows));
    moe_route_launch(e->moe_logits, rows, m.num_experts, k, m.norm_topk_prob, e->moe_ids, e->moe_scores, e->stream);
    TL_TRY(moe_experts_launch(m, xn, h, e->moe_ids, e->moe_scores, MoeExpertRows{e->moe_gate, e->moe_up, e->moe_act, e->moe_y}, out, rows,
                              e->cfg.hidden_size, e->stream));
    (void)pc;  // the MoE launches carry no in-kernel stamps: tl_engine_profile_step leaves them out of its kinds
    TL_CHECK_LAUNCH("engine MoE layer");
    return TL_OK;
}

// The routes of one decode step over `batch` rows, decided before its first launch: every layer's (plan_layer), the lm_head's, the row
// order of the weighted hand-over, and whose hand-over buffers the step uses.
struct StepRoute {
    std::vector<LayerRoute> layers;
    bool frag = false;   // rows_travel_in_fragment_order
    bool head6 = false;  // lm_head on the register-resident matmul wherever the last layer leaves weighted rows
    // per-layer hand-over buffers: the fused-GEMV rows of a dense model whose attention partials fit the per-layer workspace (per_layer),
    // or the rows of the batched-matmul step (5 .. 64) when every layer hands over inside its own buffers and slice planes (per_layer_b)
    bool per_layer = false, per_layer_b = false;
};
static StepRoute plan_step(const tl_engine *e, int batch, const AttnPlan &sp) {
    const LinearCtx &ctx = e->lin;
    StepRoute s;
    s.frag = rows_travel_in_fragment_order(ctx, ctx.shapes(e->layers[0]), batch);
    s.head6 = qmm6_takes(ctx, ctx.shape(e->head()), batch);
    const bool ws_fits = sp.n_splits == 1 || sp.partials_bytes(batch) <= e->layer_ws_bytes;
    const bool own_buffers = e->layer_act_rows > 0 && batch <= e->layer_act_rows && ws_fits;
    s.per_layer = own_buffers && gemv_takes_rows(ctx, batch);
    s.per_layer_b = own_buffers && !gemv_takes_rows(ctx, batch) && ctx.force_linear == 0 && s.head6;
    for (int l = 0; l < e->cfg.num_layers; ++l) {
        s.layers.push_back(plan_layer(ctx, ctx.shapes(e->layers[l]), batch, e->is_moe(l)));
        if (e->is_moe(l)) s.per_layer = false;  // a MoE layer reads and writes the shared buffers
        if (!s.layers.back().batched_written_once()) s.per_layer_b = false;
    }
    return s;
}

// One fused decode step over slots [0, batch); `f`: step_features(e, 0, batch).
// `sp`: the step's attention plan (prepare_step); every layer completes it with what its own projections hand over (plan_decode_launch)
static int enqueue_step(tl_engine *e, int batch, const AttnPlan &sp, const StepFeatures &f, ProfCtx *pc = nullptr) {
    const tl_engine_config &c = e->cfg;
    LinearCtx &ctx = e->lin;
    StepRoute route = plan_step(e, batch, sp);
    // A step in which a live slot carries a LoRA adapter (lora.h): every projection leaves complete bf16 rows in the shared buffers, the
    // shrink / expand launches stand around them (8 more per dense layer), and the step keeps its launch boundaries.  Its layers are
    // never batched and hand nothing over weighted, kept as slice partials or unmerged; the two residual projections add to
    // residual + delta in lora_tmp, and gate|up stores complete rows for the expand launch's SwiGLU
    const bool lora = f.lora;
    if (lora) route.per_layer = route.per_layer_b = false;
    const int lora_tiles = ceil_div(batch, LORA_TILE);
    // only a step whose hand-overs all live at addresses written once per step may be replayed without cache maintenance (tl_engine_decode)
    e->step_written_once = route.per_layer || route.per_layer_b;
    // x enters the step from the embedding gather (embed_slots_kernel / the previous step's step_end_kernel), which leaves the
    // per-row partial sums of squares in ss_x; every slice reduction that rewrites x or h refreshes them (or says it did not)
    int x_ss = QM3_SS;  // partials per row in ssx_cur (0 = none): QM3_SS from the embedding kernels, then whatever the last writer of x left
    // 5 .. 64 rows on the register-resident matmul: xw_cur holds x weighted by the NEXT RMSNorm's weight whenever xw is set (written by
    // the w_down epilogue of the previous layer, or by one pointwise launch ahead of layer 0)
    bool xw = false;
    // where the residual stream, its weighted copy and its sums of squares stand (the shared buffers, or the last layer's own in a per-layer mode)
    uint16_t *x_cur = e->shared.x_out, *xw_cur = e->shared.xn;
    float *ssx_cur = e->shared.ss_x_out;
    // a layer's hand-over buffers: the shared ones (no slice planes: the context's workspace), or -- the AQL route's per-layer modes -- its
    // own (written once per step)
    const Act &shared = e->shared;
    for (int l = 0; l < c.num_layers; ++l) {
        const tl_layer_weights &w = e->layers[l];
        const LayerRoute &rt = route.layers[l];
        // The one input of a route that is not known ahead: are the row's sums of squares there when the layer starts?  In a dense model
        // they are -- QM3_SS per row from the embedding kernels, QM3_SS or rows / 16 from a w_down that leaves weighted rows -- so this cannot
        // fire there; should it ever, the step must not be replayed as "written once" over buffers written several times
        const bool batched = !lora && rt.batched && x_ss > 0 && qmm3_takes_ss(x_ss);
        TL_REQUIRE(batched || !route.per_layer_b, "engine: a layer fell out of the batched branch of a step planned on the per-layer buffers");
        const Act &b = (batched ? route.per_layer_b : route.per_layer) ? e->layer_act[l] : shared;
        ProjResult r;
        if (batched && rt.qkv6) {
            if (!xw) {
                const long n8 = (long)batch * c.hidden_size / 8;
                hipLaunchKernelGGL(weight_rows_kernel, dim3(ceil_div(n8, 256)), dim3(256), 0, e->stream, x_cur, (const uint16_t *)w.input_norm_dev,
                                   e->shared.xn, n8, c.hidden_size / 8, route.frag ? 1 : 0);
                xw_cur = e->shared.xn;
            }
            Proj p = proj(w.wqkv, xw_cur, b.qkv, batch);
            p.ss_in = ssx_cur, p.ss_in_n = x_ss, p.frag = route.frag;
            TL_TRY(engine_qmm6(ctx, p, pc));
        } else {
            Proj p = proj(w.wqkv, x_cur, b.qkv, batch);
            p.pro = PRO_RMSNORM, p.norm_w = w.input_norm_dev, p.ss_in = x_ss ? ssx_cur : nullptr, p.ss_in_n = x_ss;
            p.keep = !lora && e->attn.knobs.qkv_partials && attn_takes_qkv_partials(c.head_dim, sp.rq);
            TL_TRY(engine_linear(ctx, p, pc, &r));
        }
        if (lora) TL_TRY(lora_group(e, l, tl_engine::LORA_QKV, e->lora_tiles_decode, lora_tiles, batch, x_cur, w.input_norm_dev, TL_LORA_ADD, nullptr, b.qkv));
        xw = false;
        AttnCall at{};
        at.qkv = b.qkv, at.q_norm = w.q_norm_dev, at.k_norm = w.k_norm_dev, at.key_pages = e->layer_k(l), at.value_pages = e->layer_v(l);
        at.key_scales = e->layer_ks(l), at.value_scales = e->layer_vs(l), at.out = b.attn, at.ws = b.attn_ws;
        at.qkv_parts = r.kept;
        const bool wo_can_merge = !lora && wo_merge_applicable(ctx, ctx.shape(w.wo), batch, sp.n_splits, c.head_dim, c.num_heads);
        const AttnPlan ap = plan_decode_launch(sp, e->attn.geometry, e->attn.knobs, sp.kv8, r.kept.partial != nullptr, wo_can_merge);
        TL_TRY(launch_decode_attention(e->attn, ap, at, batch, pc));
        const bool merge_left = ap.wo_merges();  // the wo GEMV of one row merges the attention windows itself where the plan leaves them to it
        TL_REQUIRE(!(batched && merge_left), "engine: a batched step left its attention windows unmerged");
        if (lora) TL_TRY(lora_group(e, l, tl_engine::LORA_O, e->lora_tiles_decode, lora_tiles, batch, b.attn, nullptr, TL_LORA_RESIDUAL_PRE, x_cur, e->lora_tmp));
        Proj po = proj(w.wo, b.attn, b.h, batch);
        po.epi = EPI_RESIDUAL, po.residual = lora ? e->lora_tmp : x_cur, po.kind = 1;
        if (merge_left) po.pro = PRO_ATTN_MERGE, po.merge_ws = b.attn_ws, po.n_splits = sp.n_splits;
        x_cur = b.x_out, ssx_cur = b.ss_x_out;  // where the layer leaves the residual stream
        if (e->is_moe(l)) {  // wo + residual, then the MoE MLP as its own launches (no producer-side sums for the next layer)
            TL_TRY(engine_linear(ctx, po, pc));
            TL_TRY(tl_rms_norm(b.h, w.post_norm_dev, b.xn, batch, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
            TL_TRY(engine_moe_mlp(e, l, b.xn, b.h, b.x_out, batch, pc));
            x_ss = 0;
            continue;
        }
        TL_REQUIRE(w.wgu.weight_dev != nullptr, "engine: a layer has neither a dense MLP nor experts (tl_engine_set_moe_layer)");
        // h leaves wo twice when gate|up can take it weighted (a batched layer; the GEMVs by weighted_rows_apply): as the residual
        // stream and, in xn, times the post-attention norm weight
        const bool h_weighted = !lora && (batched || rt.gemv_weighted);
        po.ss_out = b.ss_h;
        if (!lora) {
            po.norm_out = w.post_norm_dev, po.out_w = h_weighted ? b.xn : nullptr, po.frag = batched && route.frag;
            po.planes = b.planes[0], po.planes_bytes = e->layer_plane_bytes[0];
        }
        TL_TRY(batched && rt.wo6 ? engine_qmm6(ctx, po, pc, &r) : engine_linear(ctx, po, pc, &r));
        const int h_ss = r.ss_n;
        if (batched) TL_REQUIRE(h_ss > 0 && qmm3_takes_ss(h_ss), "engine: the wo projection left no sums of squares for its weighted rows");
        else if (h_weighted) TL_REQUIRE(h_ss > 0, "engine: the wo GEMV left no sums of squares for its weighted rows");
        Proj pg = proj(w.wgu, h_weighted ? b.xn : b.h, lora ? ctx.gu : b.act, batch);
        pg.epi = lora ? EPI_STORE : EPI_SWIGLU, pg.kind = 2, pg.ss_in = h_ss ? b.ss_h : nullptr, pg.ss_in_n = h_ss, pg.frag = batched && route.frag;
        if (!batched) pg.pro = h_weighted ? PRO_RMS_WEIGHTED : PRO_RMSNORM, pg.norm_w = h_weighted ? nullptr : w.post_norm_dev;
        TL_TRY(batched ? engine_qmm6(ctx, pg, pc) : engine_linear(ctx, pg, pc));
        if (lora) {
            TL_TRY(lora_group(e, l, tl_engine::LORA_GU, e->lora_tiles_decode, lora_tiles, batch, b.h, w.post_norm_dev, TL_LORA_SWIGLU, ctx.gu, b.act));
            TL_TRY(lora_group(e, l, tl_engine::LORA_DOWN, e->lora_tiles_decode, lora_tiles, batch, b.act, nullptr, TL_LORA_RESIDUAL_PRE, b.h, e->lora_tmp));
        }
        Proj pd = proj(w.wdown, b.act, b.x_out, batch);
        pd.epi = EPI_RESIDUAL, pd.residual = lora ? e->lora_tmp : b.h, pd.kind = 3, pd.ss_out = b.ss_x_out;
        if (!lora) pd.planes = b.planes[1], pd.planes_bytes = e->layer_plane_bytes[1];
        const bool x_weighted = batched && rt.down != LayerRoute::DOWN_ROUTER;
        if (x_weighted) {
            // the rows w_down leaves are weighted for their next reader: the next layer's input norm, or the final norm ahead of lm_head
            pd.norm_out = l + 1 < c.num_layers ? e->layers[l + 1].input_norm_dev : e->final_norm;
            pd.out_w = b.xw, pd.frag = route.frag;
            xw_cur = b.xw;
        }
        TL_TRY(batched && rt.down == LayerRoute::DOWN_QMM6 ? engine_qmm6(ctx, pd, pc, &r) : engine_linear(ctx, pd, pc, &r));
        x_ss = r.ss_n;
        xw = x_weighted && x_ss > 0;
    }
    ProjResult rh;
    if (xw && route.head6 && qmm3_takes_ss(x_ss)) {
        Proj ph = proj(e->head(), xw_cur, e->logits, batch);
        ph.kind = 4, ph.ss_in = ssx_cur, ph.ss_in_n = x_ss, ph.frag = route.frag;
        TL_TRY(engine_qmm6(ctx, ph, pc));
    } else {
        Proj ph = proj(e->head(), x_cur, e->logits, batch);
        ph.pro = PRO_RMSNORM, ph.norm_w = e->final_norm, ph.kind = 4, ph.ss_in = x_ss ? ssx_cur : nullptr, ph.ss_in_n = x_ss;
        ph.tile_max = e->lm_tile_max_on ? e->lm_tile_max : nullptr;
        TL_TRY(engine_linear(ctx, ph, pc, &rh));
    }
    const bool tile_max = rh.maxima_rows == batch;
    launch_logit_chain(e, e->logits, 0, batch, 0, 1, e->shared.x_out, tile_max ? e->lm_tile_max : nullptr, tile_max ? e->head().rows / 16 : 0, e->shared.ss_x_out, e->tokens, f, pc);
    TL_CHECK_LAUNCH("engine step end");
    return TL_OK;
}

// ---- the slot table (slot_table.h) on the device ---------------------------------------------------------------------------
// a refusal of the table as the engine reports it
static int table_rc(const char *why) { return why ? fail(TL_ERR_INVALID, why) : TL_OK; }

// K and V rows of one page, every layer (device to device, stream ordered)
static int copy_page(tl_engine *e, int from, int to) {
    const tl_engine_config &c = e->cfg;
    const size_t page_bytes = (size_t)c.num_kv_heads * c.page_size * c.head_dim * e->kv_elem_bytes();
    const size_t page_rows = (size_t)c.num_kv_heads * c.page_size;  // FP8 pages: one scale per row
    for (int l = 0; l < c.num_layers; ++l) {
        TL_HIP(hipMemcpyAsync((char *)e->layer_k(l) + (size_t)to * page_bytes, (char *)e->layer_k(l) + (size_t)from * page_bytes, page_bytes,
                              hipMemcpyDeviceToDevice, e->stream));
        TL_HIP(hipMemcpyAsync((char *)e->layer_v(l) + (size_t)to * page_bytes, (char *)e->layer_v(l) + (size_t)from * page_bytes, page_bytes,
                              hipMemcpyDeviceToDevice, e->stream));
        if (e->kv_format == TL_KV_FP8_E4M3) {
            TL_HIP(hipMemcpyAsync(e->layer_ks(l) + (size_t)to * page_rows, e->layer_ks(l) + (size_t)from * page_rows, page_rows * 4,
                                  hipMemcpyDeviceToDevice, e->stream));
            TL_HIP(hipMemcpyAsync(e->layer_vs(l) + (size_t)to * page_rows, e->layer_vs(l) + (size_t)from * page_rows, page_rows * 4,
                                  hipMemcpyDeviceToDevice, e->stream));
        }
    }
    return TL_OK;
}

// the pool's counters as the statistics report them (pages_in_use + pages_free + retained pages == num_pages)
static void page_stats(const SlotTable &t, tl_engine_stats *out) {
    out->pages_in_use = t.pages_in_use();
    out->pages_free = t.pages_free();
    out->peak_pages_in_use = t.peak_pages_in_use;
    out->page_allocations = t.page_allocations;
    out->reused_page_allocations = t.reused_page_allocations;
}

// The table's edits on the stream: the page copies are enqueued first (a fresh page is filled before the row entry that publishes
// it), then the block-table writes join `pk`, which the caller pokes together with the words of its own (context, live, ...).
static int apply_edits(tl_engine *e, const SlotEdits &ed, Pokes &pk) {
    const tl_engine_config &c = e->cfg;
    for (const SlotEdits::Copy &cp : ed.copies) {
        if (cp.rows == c.page_size) TL_TRY(copy_page(e, cp.from, cp.to));
        else TL_TRY(kv_copy_rows(e->kv_pools_dev, e->kv_pools_n, c.num_kv_heads, c.page_size, cp.from, cp.to, cp.rows, e->stream));
    }
    for (const SlotEdits::Row &r : ed.rows) pk.emplace_back(e->block_table + (size_t)r.slot * c.max_pages_per_seq + r.index, r.page);
    return TL_OK;
}

static int slot_check(const tl_engine *e, int slot, bool must_be_live) {
    if (!e) return fail(TL_ERR_INVALID, "engine: null engine");
    return table_rc(e->table.check(slot, must_be_live));
}
// ... for the calls that read or write the slot's K/V: a parked slot has none on the device (tl_engine_unpark first)
static int slot_check_unparked(const tl_engine *e, int slot) {
    if (!e) return fail(TL_ERR_INVALID, "engine: null engine");
    return table_rc(e->table.check_unparked(slot));
}
// ... for the calls that feed the slot tokens (prefill, packed prefill, verify, score, embed): a slot a stop has frozen takes none
// until tl_engine_set_stop resumes it; what an earlier call's stop launch decided is read first
static int slot_check_feeds(tl_engine *e, int slot) {
    if (!e) return fail(TL_ERR_INVALID, "engine: null engine");
    TL_TRY(stop_reconcile(e));
    TL_TRY(table_rc(e->table.check_unparked(slot)));
    if (e->table.slots[slot].stopped) return fail(TL_ERR_INVALID, "engine: the slot has stopped (tl_engine_set_stop re-arms or disarms it first)");
    return TL_OK;
}

// fork / move (move = true), behind the table's: the pending input token travels on the device, and the record says what else does
static int settings_carry(tl_engine *e, int src, int dst, bool move, Pokes &pk) {
    TL_HIP(hipMemcpyAsync(e->tokens + dst, e->tokens + src, sizeof(int32_t), hipMemcpyDeviceToDevice, e->stream));
    SettingsEdits ed;
    e->settings.carry(src, dst, move, ed);
    return settings_apply(e, ed, pk);
}

}  // namespace tl

// ================================================================================================
// ---- the engine's memory (engine_layout.h) -------------------------------------------------------------------------------------------------
static_assert(POOL_MAX_SEQS == PACKED_MAX_SEQS, "pool.h takes the sequences of a packed pass");
static_assert(VA_MAX_ROWS == VERIFY_BATCH_ROWS && VA_MAX_LEN == VERIFY_MAX_LEN, "verify_attn_host.h and the layout size one pass");
static_assert(sizeof(tl_engine::SpecRecord::proposal) == VERIFY_MAX_LEN * sizeof(int32_t), "SpecRecord holds the rows of one tl_engine_verify_sampled");
static_assert(tl_engine::VerifyScratch::DESC_ARRAYS == VERIFY_DESC_ARRAYS, "the layout sizes `desc` by its arrays");

// what the layouts ask of the device headers and of the engine as it stands (matmul_ws_need: verify_alloc's own)
static LayoutInputs layout_inputs(const tl_engine *e) {
    LayoutInputs in;
    in.attn_ws_bytes = e->attn.ws_bytes, in.attn_ws_pad = ATTN_WS_PAD, in.qm3_ss = QM3_SS;
    in.plane_bytes[0] = e->layer_plane_bytes[0], in.plane_bytes[1] = e->layer_plane_bytes[1];
    in.matmul_ws_engine = e->lin.splitk_ws_bytes, in.aql = e->aql_on, in.ring_cap = e->ring_cap, in.tile_max_bytes = sizeof(f32x2);
    in.verify_ws_rows = verify_ws_rows(e->cfg.num_heads), in.verify_head_dim = VA_D, in.verify_result_bytes = sizeof(tl_verify_result);
    in.moe_k = e->moe_k_max, in.moe_e = e->moe_e_max, in.moe_i = e->moe_i_max;
    return in;
}

// Bytes the matmuls of the engine's matrices need of the router's workspace: the fp32 slice partials of the skinny matmul's plans at
// s0 .. s1 rows and the split-K partials of the GEMM at g0 .. g1 rows, over the five matrix shapes (the first layer that has a dense MLP
// sizes the MLP's) and, with `routers`, the MoE routers
static size_t matmul_ws_need(const tl_engine *e, int s0, int s1, int g0, int g1, bool routers) {
    const tl_layer_weights *dense = &e->layers[0];
    for (const auto &l : e->layers)
        if (l.wgu.weight_dev) {
            dense = &l;
            break;
        }
    std::vector<tl_w4> mats = {e->layers[0].wqkv, e->layers[0].wo, dense->wgu, dense->wdown, e->head()};
    for (int l = 0; routers && l < e->cfg.num_layers; ++l)
        if (e->is_moe(l)) mats.push_back(e->moe[l].router);
    size_t need = 0;
    for (const tl_w4 &w : mats) {
        if (!w.weight_dev) continue;
        for (int M = s0; M <= s1; ++M) {
            const Qmm3Plan p3 = qmm3_plan(M, w.cols, w.rows, -1, e->lin.ncu);
            if (p3.ok) need = std::max(need, p3.partial_bytes);
        }
        for (int M = g0; M <= g1; ++M) need = std::max(need, tl_quantized_matmul_workspace_bytes(M, w.cols, w.rows, TL_BF16, 1, 1));
    }
    return need;
}

// ---- the steps of tl_engine_create_kv, in the order it takes them ----------------------------------------------------------------
// the K / V page pools of every layer (FP8 pages: their row scales beside them), zeroed
static int create_kv_pools(tl_engine *e) {
    const tl_engine_config &c = e->cfg;
    e->layer_pool_elems = (size_t)c.num_pages * c.num_kv_heads * c.page_size * c.head_dim;
    const size_t pool_bytes = e->layer_pool_elems * e->kv_elem_bytes() * c.num_layers;
    TL_TRY(e->kv_mem[0].alloc(pool_bytes, "engine_create: hipMalloc(key pages) failed"));
    TL_TRY(e->kv_mem[1].alloc(pool_bytes, "engine_create: hipMalloc(value pages) failed"));
    e->kpool = e->kv_mem[0].at<uint16_t>(), e->vpool = e->kv_mem[1].at<uint16_t>();
    e->kv_bytes = 2 * pool_bytes;
    if (e->kv_format == TL_KV_FP8_E4M3) {
        // one float32 scale per (page, kv head, slot) row; zero like the codes (a zero scale times a zero code is the zero the bf16 pool holds)
        e->layer_scale_elems = (size_t)c.num_pages * c.num_kv_heads * c.page_size;
        const size_t scale_bytes = e->layer_scale_elems * 4 * c.num_layers;
        TL_TRY(e->kv_mem[2].alloc(scale_bytes, "engine_create: hipMalloc(key scales) failed"));
        TL_TRY(e->kv_mem[3].alloc(scale_bytes, "engine_create: hipMalloc(value scales) failed"));
        e->kscale_pool = e->kv_mem[2].at<float>(), e->vscale_pool = e->kv_mem[3].at<float>();
        if (hipMemsetAsync(e->kscale_pool, 0, scale_bytes, e->stream) != hipSuccess ||
            hipMemsetAsync(e->vscale_pool, 0, scale_bytes, e->stream) != hipSuccess)
            return fail(TL_ERR_HIP, "engine_create: memset(KV scales) failed");
        e->kv_bytes += 2 * scale_bytes;
    }
    // Masked (out-of-context) token slots are still loaded and multiplied by a zero weight in the decode kernel,
    // so the pools must never hold NaN/Inf bit patterns: start from zeros (kernels only ever write finite values).
    if (hipMemsetAsync(e->kpool, 0, pool_bytes, e->stream) != hipSuccess ||
        hipMemsetAsync(e->vpool, 0, pool_bytes, e->stream) != hipSuccess)
        return fail(TL_ERR_HIP, "engine_create: memset(KV pools) failed");
    return TL_OK;
}

// the per-layer decode activations of the AQL route (engine_layout.h LayerLayout), zeroed
static int create_layer_acts(tl_engine *e) {
    const tl_engine_config &c = e->cfg;
    const int q_dim = e->q_dim();
    // slice planes of the sliced matmuls a batched step can take (wo, w_down), the largest over 5 .. rows rows
    for (int M = std::min(5, e->lin.qmm3_min_rows); M <= layer_act_rows(c.max_batch); ++M) {
        const Qmm3Plan pw = qmm3_plan(M, q_dim, c.hidden_size, -1, e->lin.ncu), pd = qmm3_plan(M, c.intermediate_size, c.hidden_size, -1, e->lin.ncu);
        if (pw.ok) e->layer_plane_bytes[0] = std::max(e->layer_plane_bytes[0], align_up(pw.partial_bytes, 256));
        if (pd.ok) e->layer_plane_bytes[1] = std::max(e->layer_plane_bytes[1], align_up(pd.partial_bytes, 256));
    }
    const LayerLayout ll = layer_layout(c, layout_inputs(e));
    e->layer_act_bytes = ll.bytes * c.num_layers;
    TL_TRY(e->layer_act_mem.alloc(e->layer_act_bytes, "engine_create: hipMalloc(per-layer decode activations) failed"));
    if (hipMemsetAsync(e->layer_act_mem.at(), 0, e->layer_act_bytes, e->stream) != hipSuccess)
        return fail(TL_ERR_HIP, "engine_create: hipMalloc(per-layer decode activations) failed");
    for (int l = 0; l < c.num_layers; ++l) e->layer_act.push_back(layer_act(e->layer_act_mem.at(), ll, l));
    e->layer_act_rows = ll.rows;
    e->layer_ws_bytes = ll[LayerLayout::PLANE0].off - ll[LayerLayout::ATTN_WS].off;  // (the piece, rounded up like every piece)
    return TL_OK;
}

// RoPE table for every position a sequence can reach, and the slots' current rows
static int create_rope_tables(tl_engine *e) {
    const tl_engine_config &c = e->cfg;
    const long max_pos = std::min<long>((long)c.max_pages_per_seq * c.page_size + 1, 1 << 20);
    e->rope_positions = (int)max_pos;
    const int half = c.head_dim / 2;
    TL_TRY(e->rope_table_mem.alloc((size_t)max_pos * half * sizeof(float2), "engine_create: hipMalloc(rope table) failed"));
    e->rope_table = e->rope_table_mem.at<float2>();
    hipLaunchKernelGGL(rope_table_kernel, dim3(ceil_div(max_pos * half, 256)), dim3(256), 0, e->stream, e->rope_table,
                       (int)max_pos, half, c.rope_theta);
    if (hipGetLastError() != hipSuccess) return fail(TL_ERR_HIP, "engine_create: rope table kernel failed");
    TL_TRY(e->rope_cur_mem.alloc((size_t)c.max_batch * half * sizeof(float2), "engine_create: hipMalloc(rope state) failed"));
    e->rope_cur = e->rope_cur_mem.at<float2>(), e->attn.rope_cur = e->rope_cur;
    if (hipMemsetAsync(e->rope_cur, 0, (size_t)c.max_batch * half * sizeof(float2), e->stream) != hipSuccess)
        return fail(TL_ERR_HIP, "engine_create: hipMalloc(rope state) failed");
    return TL_OK;
}

static int create_weight_copies(tl_engine *e) {
    const tl_engine_config &c = e->cfg;
    // decode-path weight copies in the tiled MFMA layout
    {
        auto add_tiled = [&](const tl_w4 &w) -> bool {
            if (w.rows % 16 != 0 || w.cols % 128 != 0 || e->lin.tiled.count(w.weight_dev)) return true;
            const char *failed = "engine_create: hipMalloc(tiled weights) failed";
            e->tiled_mem.emplace_back();
            if (tiled_w4_make(w, e->stream, e->tiled_mem.back(), e->lin.tiled[w.weight_dev], failed, failed) != TL_OK) return false;
            e->tiled_bytes += (size_t)w.rows * w.cols / 2 + (size_t)w.rows * (w.cols / 128) * 4;
            return true;
        };
        bool ok = true;
        for (const auto &l : e->layers) {
            ok = ok && add_tiled(l.wqkv) && add_tiled(l.wo);
            if (l.wgu.weight_dev) ok = ok && add_tiled(l.wgu) && add_tiled(l.wdown);
        }
        ok = ok && add_tiled(e->head());
        if (!ok) return fail(TL_ERR_HIP, "engine_create: hipMalloc(tiled weights) failed");
    }
    if (c.max_prefill_rows >= GEMM8_MIN_ROWS) {  // the caller asked for chunks the plain bf16 GEMM takes: expand the layer matrices once
        auto add_bf16 = [&](const tl_w4 &w) -> bool {
            if (!w.weight_dev || w.cols % 128 != 0 || e->lin.bf16w.count(w.weight_dev) || !gemm8_applicable(c.max_prefill_rows, w.rows, w.cols)) return true;
            const size_t bytes = (size_t)w.rows * w.cols * 2;
            DeviceBlock copy;
            if (copy.alloc(bytes, "engine_create: hipMalloc(bf16 weights for the prefill GEMM) failed") != TL_OK) return false;
            uint16_t *wb = copy.at<uint16_t>();
            if (dequant_w4_to_bf16(w.weight_dev, (const uint16_t *)w.scales_dev, (const uint16_t *)w.biases_dev, wb, w.rows, w.cols, e->stream) != 0) return false;
            e->bf16w_mem.push_back(std::move(copy));
            e->lin.bf16w[w.weight_dev] = wb;
            e->bf16w_bytes += bytes;
            return true;
        };
        bool ok = true;
        for (const auto &l : e->layers) {
            ok = ok && add_bf16(l.wqkv) && add_bf16(l.wo);
            if (l.wgu.weight_dev) ok = ok && add_bf16(l.wgu) && add_bf16(l.wdown);
        }
        if (!ok) return fail(TL_ERR_HIP, "engine_create: hipMalloc(bf16 weights for the prefill GEMM) failed");
    }
    return TL_OK;
}

extern "C" int tl_engine_create(const tl_engine_config *cfg, const tl_layer_weights *layers, const tl_w4 *embed,
                                const void *final_norm_dev, const tl_w4 *lm_head, void *stream, tl_engine **out) {
    return tl_engine_create_kv(cfg, layers, embed, final_norm_dev, lm_head, stream, TL_KV_BF16, out);
}

extern "C" int tl_engine_create_kv(const tl_engine_config *cfg, const tl_layer_weights *layers, const tl_w4 *embed,
                                   const void *final_norm_dev, const tl_w4 *lm_head, void *stream, int kv_format, tl_engine **out) {
    TL_REQUIRE(cfg && layers && embed && final_norm_dev && out, "engine_create: null argument");
    const tl_engine_config &c = *cfg;
    TL_REQUIRE(kv_format == TL_KV_BF16 || kv_format == TL_KV_FP8_E4M3, "engine_create: kv_format must be TL_KV_BF16 or TL_KV_FP8_E4M3");
    TL_REQUIRE(kv_format == TL_KV_BF16 || c.head_dim == 128, "engine_create: FP8 KV pages need head_dim 128");
    TL_REQUIRE(c.num_layers > 0 && c.hidden_size > 0 && c.hidden_size % 128 == 0, "engine_create: hidden_size must be a positive multiple of 128");
    TL_REQUIRE(c.num_heads > 0 && c.num_kv_heads > 0 && c.num_heads % c.num_kv_heads == 0,
               "engine_create: num_heads must be divisible by num_kv_heads");
    TL_REQUIRE(c.head_dim == 32 || c.head_dim == 64 || c.head_dim == 128, "engine_create: head_dim must be 32, 64 or 128");
    TL_REQUIRE((c.num_heads * c.head_dim) % 128 == 0 && c.intermediate_size % 128 == 0,
               "engine_create: projection widths must be multiples of the quantization group (128)");
    TL_REQUIRE(c.page_size > 0 && c.num_pages > 0 && c.max_batch > 0 && c.max_batch <= 256 && c.max_pages_per_seq > 0,
               "engine_create: need page_size, num_pages, max_pages_per_seq > 0 and 1 <= max_batch <= 256");
    TL_REQUIRE(c.max_prefill_rows > 0, "engine_create: max_prefill_rows must be positive");
    const int qkv_dim = (c.num_heads + 2 * c.num_kv_heads) * c.head_dim;
    const int q_dim = c.num_heads * c.head_dim;
    for (int l = 0; l < c.num_layers; ++l) {
        TL_TRY(check_w4(layers[l].wqkv, qkv_dim, c.hidden_size, "wqkv"));
        TL_TRY(check_w4(layers[l].wo, c.hidden_size, q_dim, "wo"));
        // a layer without a dense MLP (both null) must get its experts through tl_engine_set_moe_layer before the first step
        if (layers[l].wgu.weight_dev != nullptr || layers[l].wdown.weight_dev != nullptr) {
            TL_TRY(check_w4(layers[l].wgu, 2 * c.intermediate_size, c.hidden_size, "wgu"));
            TL_TRY(check_w4(layers[l].wdown, c.hidden_size, c.intermediate_size, "wdown"));
        }
        TL_REQUIRE(layers[l].input_norm_dev && layers[l].post_norm_dev && layers[l].q_norm_dev && layers[l].k_norm_dev,
                   "engine_create: null norm weight");
    }
    TL_TRY(check_w4(*embed, c.vocab_size, c.hidden_size, "embed_tokens"));
    if (lm_head) TL_TRY(check_w4(*lm_head, c.vocab_size, c.hidden_size, "lm_head"));

    // a failure below tears the partly built engine down like any other: tl_engine_destroy, and with it every block it holds so far
    std::unique_ptr<tl_engine, void (*)(tl_engine *)> owner(new tl_engine(), tl_engine_destroy);
    tl_engine *e = owner.get();
    e->cfg = c;
    e->kv_format = kv_format;
    if (hipGetDevice(&e->device) != hipSuccess) return fail(TL_ERR_HIP, "engine_create: hipGetDevice failed");
    e->layers.assign(layers, layers + c.num_layers);
    e->embed = *embed;
    if (lm_head) e->lm_head = *lm_head;
    e->final_norm = final_norm_dev;
    e->stream = (hipStream_t)stream;
    if (!e->stream) {
        // The legacy default stream cannot be captured into a graph: own a non-blocking stream instead, and
        // make sure everything the caller enqueued before (weight uploads / re-packing) has finished.
        if (hipDeviceSynchronize() != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
            return fail(TL_ERR_HIP, "engine_create: could not create the engine stream");
        e->owned_stream.s = e->stream;
    }
    e->rows_cap = prefill_rows(c);

    // ---- the arena (engine_layout.h): its attention partials first -- decode (batch*Hq rows x 64 splits) or the L<=8 operator path during
    // short prefills (the decode partials: attn_plan.h, attn_partials_capacity)
    e->attn.geometry = AttnGeometry{c.num_heads, c.num_kv_heads, c.head_dim, c.page_size, c.max_pages_per_seq};
    e->attn.eps = c.rms_norm_eps, e->attn.rope_theta = c.rope_theta, e->attn.stream = e->stream;
    e->attn.ws_bytes = attn_partials_capacity(e->attn.geometry, c.max_batch);
    for (int L = 1; L <= c.max_prefill_rows; ++L)  // the paged attention operator may split the context for any chunk length
        e->attn.ws_bytes = std::max(e->attn.ws_bytes, tl_paged_attention_workspace_bytes(c.num_heads, L, c.head_dim, c.page_size,
                                                                                       c.max_pages_per_seq, c.num_heads,
                                                                                       c.num_kv_heads, 0));
    const ArenaLayout al = arena_layout(c, layout_inputs(e));
    e->arena_bytes = al.bytes, e->arena_act_off = al.act_off;

    TL_TRY(e->arena.alloc(e->arena_bytes, "engine_create: hipMalloc(arena) failed"));
    // sampling parameters per slot (all zero: greedy): seeds first for their 8-byte alignment
    e->settings.init(settings_sizes(e));
    TL_TRY(settings_blocks(e, 1u << SB_SAMPLE));
    TL_TRY(create_kv_pools(e));

    {
        using A = ArenaLayout;
        char *m = e->arena.at();
        e->block_table = piece_at<int32_t>(m, al[A::BLOCK_TABLE]), e->context_lens = piece_at<int32_t>(m, al[A::CONTEXT_LENS]);
        e->attn.block_table = e->block_table, e->attn.context_lens = e->context_lens;
        e->tokens = piece_at<int32_t>(m, al[A::TOKENS]), e->live = piece_at<int32_t>(m, al[A::LIVE]), e->produced = piece_at<int32_t>(m, al[A::PRODUCED]);
        e->ring = piece_at<int32_t>(m, al[A::RING]), e->scratch_ctx = piece_at<int32_t>(m, al[A::SCRATCH_CTX]);
        e->prefill_tokens = piece_at<int32_t>(m, al[A::PREFILL_TOKENS]);
        e->shared = arena_act(m, al);
        e->lin.xn = e->shared.xn, e->lin.tmp = piece_at<uint16_t>(m, al[A::TMP]), e->lin.gu = piece_at<uint16_t>(m, al[A::GU]);
        e->q_t = piece_at<uint16_t>(m, al[A::Q_T]), e->attn_t = piece_at<uint16_t>(m, al[A::ATTN_T]), e->logits = piece_at<uint16_t>(m, al[A::LOGITS]);
        e->verify_ids = piece_at<int32_t>(m, al[A::VERIFY_IDS]), e->lm_tile_max = piece_at<f32x2>(m, al[A::LM_TILE_MAX]);
    }
    e->lin.stream = e->stream, e->lin.rms_norm_eps = c.rms_norm_eps;
    e->lin.ncu = qmm3_num_cus();
    e->lin.read_env();
    e->attn.knobs.read_env();
    // Decode steps replay as AQL packets on the engine's own HSA queue (aql.h) unless TL_AQL=0: the same captured step, without the
    // cache maintenance HIP puts between its launches (0.987 -> 0.929 ms per token at Qwen3-4B, logits bit-identical).  Where the route is
    // not available (no code objects next to the library, no HSA agent for the device) the engine stays on hipGraphLaunch and says why
    // in tl_engine_replay_route(); TL_AQL=1 makes that an error instead.
    const char *aql_env = getenv("TL_AQL");
    if (aql_env == nullptr || atoi(aql_env) != 0) {
        {
            AqlRuntime &rt = AqlRuntime::for_device(e->device);
            e->aql_rt = &rt;
            std::string why;
            e->aql_queue = std::make_unique<AqlQueue>();
            if (!rt.ensure_loaded(library_dir()) || !e->aql_queue->create(rt, why)) {
                e->aql_why = rt.ok() ? why : rt.why();
                e->aql_queue.reset();
                if (aql_env != nullptr) {
                    return fail(TL_ERR_UNSUPPORTED, "engine_create: TL_AQL=1 but the AQL route is not available: " + e->aql_why);
                }
            }
        }
        if (e->aql_queue) {
            e->aql_on = true;
            // the route's code objects are compiled with TL_COHERENT (common.h): no cache maintenance between the launches of a step.
            // (tl_engine_set_option "aql_fences" = 1 puts HIP's agent-scope fences back on every packet: the A/B of what the maintenance costs)
            e->aql_fences.inner_acquire = e->aql_fences.inner_release = HSA_FENCE_SCOPE_NONE;
            // per-layer decode activations (1-4 rows: the fused-GEMV step; 5-64 rows since round 5: the batched-matmul step): every hand-over
            // address of a step is written once per step.  The attention partials hold 16 windows per row (at most 1,024 row-windows): a plan
            // beyond that keeps the shared buffers and the graph route.
            TL_TRY(create_layer_acts(e));
        }
    }

    // state words: zero everything up to the activations, then the block table to -1
    if (hipMemsetAsync(e->arena.at(), 0, al.act_off, e->stream) != hipSuccess) return fail(TL_ERR_HIP, "engine_create: memset failed");
    const int bt_n = c.max_batch * c.max_pages_per_seq;
    hipLaunchKernelGGL(fill_i32_kernel, dim3(ceil_div(bt_n, 256)), dim3(256), 0, e->stream, e->block_table, -1, bt_n);
    if (hipGetLastError() != hipSuccess) return fail(TL_ERR_HIP, "engine_create: block-table init failed");

    TL_TRY(create_rope_tables(e));

    TL_TRY(create_weight_copies(e));

    {
        // Workspace of every matmul the engine can launch, allocated once: fp32 slice partials of the skinny matmul
        // (qmm3_min_rows .. 64 decode rows, any of the five matrices) and split-K partials of the prefill GEMM (9 ..
        // rows_cap rows).  Graphs captured later hold this address, so it is never reallocated.
        const size_t need = matmul_ws_need(e, 1, std::min(64, e->rows_cap), 9, e->rows_cap, false);
        if (need > 0) {
            TL_TRY(e->splitk_mem.alloc(need, "engine_create: hipMalloc(matmul workspace) failed"));
            e->lin.splitk_ws = e->splitk_mem.at<void>(), e->lin.splitk_ws_bytes = need;
        }
    }

    e->moe.assign(c.num_layers, tl_moe_weights{});
    e->table.init(c.max_batch, c.num_pages, c.page_size, c.max_pages_per_seq);  // (the pool hands out 0, 1, 2, ...)
    e->stats.kv_bytes = e->kv_bytes;
    e->stats.workspace_bytes = e->arena_bytes + e->tiled_bytes + e->bf16w_bytes;
    *out = owner.release();
    return TL_OK;
}

extern "C" int tl_engine_set_moe_layer(tl_engine *e, int layer, const tl_moe_weights *w) {
    TL_REQUIRE(e && w, "engine_set_moe_layer: null argument");
    const tl_engine_config &c = e->cfg;
    TL_REQUIRE(layer >= 0 && layer < c.num_layers, "engine_set_moe_layer: layer out of range");
    TL_REQUIRE(e->plans.empty() && e->stats.decode_steps == 0 && e->stats.prefill_tokens == 0,
               "engine_set_moe_layer: call it before the first prefill / decode");
    TL_REQUIRE(w->num_experts > 0 && w->num_experts <= 1024 && w->experts_per_token > 0 && w->experts_per_token <= 16 &&
                   w->experts_per_token <= w->num_experts,
               "engine_set_moe_layer: need 1 <= experts_per_token <= min(16, num_experts) and num_experts <= 1024");
    TL_REQUIRE(w->intermediate_size > 0 && w->intermediate_size % 128 == 0, "engine_set_moe_layer: intermediate_size must be a positive multiple of 128");
    TL_TRY(check_w4(w->router, w->num_experts, c.hidden_size, "moe router"));
    TL_REQUIRE(w->gate_dev && w->up_dev && w->down_dev && w->gate_scales_dev && w->gate_biases_dev && w->up_scales_dev &&
                   w->up_biases_dev && w->down_scales_dev && w->down_biases_dev,
               "engine_set_moe_layer: null expert tensor");
    TL_REQUIRE((long)e->rows_cap * w->experts_per_token <= 65535, "engine_set_moe_layer: max_prefill_rows x experts_per_token must stay below 65536 (one grouped launch)");
    // the router's matmul must fit the workspace sized at tl_engine_create (it does for every E <= the widest projection)
    for (int M : {1, 8, 9, e->rows_cap})
        TL_REQUIRE(tl_quantized_matmul_workspace_bytes(std::min(M, e->rows_cap), c.hidden_size, w->num_experts, TL_BF16, 1, 1) <= e->lin.splitk_ws_bytes,
                   "engine_set_moe_layer: the router matmul does not fit the engine's matmul workspace");
    const int k = std::max(e->moe_k_max, w->experts_per_token), E = std::max(e->moe_e_max, w->num_experts),
              I = std::max(e->moe_i_max, w->intermediate_size);
    if (k != e->moe_k_max || E != e->moe_e_max || I != e->moe_i_max) {  // (re)size the workspace: nothing captured holds it yet
        LayoutInputs in = layout_inputs(e);
        in.moe_k = k, in.moe_e = E, in.moe_i = I;
        const MoeLayout ml = moe_layout(c, in);
        TL_HIP(hipStreamSynchronize(e->stream));
        // (the text TL_HIP gave the hipMalloc that stood here)
        TL_TRY(e->moe_ws.alloc(ml.bytes, "hipMalloc((void **)&e->moe_ws, carve.off): " + std::string(hipGetErrorString(hipErrorOutOfMemory))));
        e->moe_ws_bytes = ml.bytes;
        char *m = e->moe_ws.at();
        e->moe_logits = piece_at<uint16_t>(m, ml[MoeLayout::LOGITS]), e->moe_ids = piece_at<int32_t>(m, ml[MoeLayout::IDS]);
        e->moe_scores = piece_at<uint16_t>(m, ml[MoeLayout::SCORES]), e->moe_gate = piece_at<uint16_t>(m, ml[MoeLayout::GATE]);
        e->moe_up = piece_at<uint16_t>(m, ml[MoeLayout::UP]), e->moe_act = piece_at<uint16_t>(m, ml[MoeLayout::ACT]);
        e->moe_y = piece_at<uint16_t>(m, ml[MoeLayout::Y]);
        e->moe_k_max = k, e->moe_e_max = E, e->moe_i_max = I;
        e->stats.workspace_bytes = e->arena_bytes + e->tiled_bytes + e->moe_ws_bytes;
    }
    e->moe[layer] = *w;
    // a model with a sparse layer never takes the per-layer decode buffers (enqueue_step: its steps stay on the shared buffers and the
    // hipGraph route): give the 17 MB per layer back (nothing captured holds them yet -- checked above)
    if (e->layer_act_mem) {
        TL_HIP(hipStreamSynchronize(e->stream));
        e->layer_act_mem.reset();
        e->layer_act.clear();
        e->layer_act_rows = 0, e->layer_act_bytes = 0, e->layer_ws_bytes = 0;
        e->layer_plane_bytes[0] = e->layer_plane_bytes[1] = 0;
    }
    return TL_OK;
}

// Test / lab hook (header): routes that have an A/B twin, switched per engine before its first step.
extern "C" int tl_engine_set_option(tl_engine *e, const char *name, int value) {
    TL_REQUIRE(e && name, "engine_set_option: null argument");
    TL_REQUIRE(e->plans.empty() && e->stats.decode_steps == 0 && e->stats.prefill_tokens == 0,
               "engine_set_option: call it before the first prefill / decode (captured steps hold the routes they were captured with)");
    const std::string n = name;
    const bool on = value != 0;
    if (n == "qmm3") e->lin.use_qmm3 = on;
    else if (n == "qmm6") e->lin.use_qmm6 = on;
    else if (n == "qmm7") e->lin.use_qmm7 = on;
    else if (n == "attn_qkv_partials") e->attn.knobs.qkv_partials = on;
    else if (n == "lmhead_tile_max") e->lm_tile_max_on = on;
    else if (n == "gemm_fused_epilogue") e->lin.gemm_fused_epilogue = on;
    else if (n == "gemm8") e->lin.use_gemm8 = on;
    else if (n == "prefill_reduce_norm") e->lin.fuse_reduce_norm = on;
    else if (n == "aql_fences") e->aql_fences.inner_acquire = e->aql_fences.inner_release = on ? HSA_FENCE_SCOPE_AGENT : HSA_FENCE_SCOPE_NONE;
    else return fail(TL_ERR_INVALID, "engine_set_option: unknown option '" + n + "' (qmm3, qmm6, qmm7, gemm8, prefill_reduce_norm, attn_qkv_partials, lmhead_tile_max, gemm_fused_epilogue, aql_fences)");
    return TL_OK;
}

extern "C" void tl_engine_destroy(tl_engine *e) {
    if (!e) return;
    (void)aql_drain(e);
    (void)hipStreamSynchronize(e->stream);
    e->plans.clear();  // (the executable graphs go while their stream still exists)
    delete e;  // the queue, every DeviceBlock, then the stream the engine created (tl_engine's member order)
}

extern "C" int tl_engine_kv_format(const tl_engine *e) { return e ? e->kv_format : TL_KV_BF16; }

extern "C" const char *tl_engine_replay_route(const tl_engine *e) {
    static thread_local std::string text;
    if (!e) return "";
    text = replay_route_text(e->aql_on, e->aql_why, step_features(e, 0, e->cfg.max_batch));
    return text.c_str();
}

extern "C" int tl_engine_synchronize(tl_engine *e) {
    TL_REQUIRE(e, "engine_synchronize: null engine");
    TL_HIP(hipStreamSynchronize(e->stream));
    return TL_OK;
}

extern "C" int tl_engine_begin(tl_engine *e, int slot) {
    TL_REQUIRE(e, "engine: null engine");
    TL_TRY(table_rc(e->table.begin(slot)));
    Pokes pk;
    pk.emplace_back(e->live + slot, 1);
    pk.emplace_back(e->context_lens + slot, 0);
    pk.emplace_back(e->produced + slot, 0);
    pk.emplace_back(e->tokens + slot, 0);
    SettingsEdits sed;
    e->settings.reset(slot, sed);
    return settings_apply(e, sed, pk);
}

extern "C" int tl_engine_reserve(tl_engine *e, int slot, int total_tokens) {
    TL_TRY(slot_check_unparked(e, slot));
    TL_REQUIRE(total_tokens >= 0, "engine_reserve: total_tokens must be nonnegative");
    SlotEdits ed;
    Pokes pk;
    TL_TRY(table_rc(e->table.reserve(slot, total_tokens, ed)));
    TL_TRY(apply_edits(e, ed, pk));
    return poke(e, pk);
}

extern "C" int tl_engine_release(tl_engine *e, int slot) {
    TL_REQUIRE(e, "engine: null engine");
    SlotEdits ed;
    Pokes pk;
    TL_TRY(table_rc(e->table.release(slot, ed)));
    TL_TRY(apply_edits(e, ed, pk));
    pk.emplace_back(e->live + slot, 0);
    pk.emplace_back(e->context_lens + slot, 0);
    pk.emplace_back(e->tokens + slot, 0);
    SettingsEdits sed;
    e->settings.reset(slot, sed);
    return settings_apply(e, sed, pk);
}

extern "C" int tl_engine_rewind(tl_engine *e, int slot, int n) {
    TL_TRY(slot_check_unparked(e, slot));
    TL_TRY(table_rc(e->settings.refuses_rewind(slot)));
    TL_TRY(lookup_catch_up(e, slot));  // (an armed slot's history first reaches the context it is rewound from)
    SlotEdits ed;
    Pokes pk;
    const int from = e->table.slots[slot].ctx;
    TL_TRY(table_rc(e->table.rewind(slot, n, ed)));
    e->settings.rewound(slot);
    const bool pending_stored = e->settings.lookup_rewound(slot, from, e->table.slots[slot].ctx);
    TL_TRY(apply_edits(e, ed, pk));  // the copy of a shared tail page before the row entry that publishes the fresh page
    pk.emplace_back(e->context_lens + slot, e->table.slots[slot].ctx);
    TL_TRY(poke(e, pk));
    return pending_stored ? lookup_store_pending(e, slot) : (int)TL_OK;
}

// Fork: slot `dst` becomes a second sequence with the same prefix as `src` (reference KvPrefixGenerator fork / restore on
// dense caches, agent/branching.py:42-208; here on the page pool).  Full pages are shared by reference count -- they are
// never written again -- and a partially filled tail page is copied, so both sequences can append independently.
extern "C" int tl_engine_fork(tl_engine *e, int src, int dst) {
    TL_REQUIRE(e, "engine: null engine");
    TL_TRY(stop_reconcile(e));
    if (!e->table.check(src, true)) TL_TRY(lookup_catch_up(e, src));  // (the ring does not travel: an armed slot's history row is complete first)
    SlotEdits ed;
    Pokes pk;
    TL_TRY(table_rc(e->table.fork(src, dst, ed)));
    TL_TRY(apply_edits(e, ed, pk));
    pk.emplace_back(e->live + dst, e->table.slots[dst].stopped ? 0 : 1);  // (a stopped sequence's copy is stopped: no sequence to a step)
    pk.emplace_back(e->context_lens + dst, e->table.slots[dst].ctx);
    pk.emplace_back(e->produced + dst, 0);
    TL_TRY(settings_carry(e, src, dst, false, pk));
    return lookup_store_pending(e, dst);
}

// the device table of every K / V (and scale) pool, built once by the first call that needs it (prefix cache, swap space): pool
// addresses never change after creation
static int ensure_pool_table(tl_engine *e) {
    if (e->kv_pools_dev) return TL_OK;
    const tl_engine_config &c = e->cfg;
    std::vector<tl_kv_pool_desc> pools;
    for (int l = 0; l < c.num_layers; ++l) {
        pools.push_back({e->layer_k(l), (size_t)c.head_dim * e->kv_elem_bytes()});
        pools.push_back({e->layer_v(l), (size_t)c.head_dim * e->kv_elem_bytes()});
        if (e->kv_format == TL_KV_FP8_E4M3) {
            pools.push_back({e->layer_ks(l), sizeof(float)});
            pools.push_back({e->layer_vs(l), sizeof(float)});
        }
    }
    TL_TRY(alloc_filled(e->kv_pools_mem, pools.size() * sizeof(tl_kv_pool_desc), "engine: hipMalloc(pool table) failed", [&](char *m) -> int {
        const hipError_t rc = hipMemcpy(m, pools.data(), pools.size() * sizeof(tl_kv_pool_desc), hipMemcpyHostToDevice);
        return rc == hipSuccess ? TL_OK : fail(TL_ERR_HIP, std::string("engine: hipMemcpy(pool table): ") + hipGetErrorString(rc));
    }));
    e->kv_pools_dev = e->kv_pools_mem.at<tl_kv_pool_desc>();
    e->kv_pools_n = (int)pools.size();
    e->kv_pools_host = std::move(pools);
    return TL_OK;
}

// ---- prefix cache (include/tinyllm_engine.h "Prefix cache"; the index is prefix_cache.h, the tail copy kv_copy.h) ----------------------
extern "C" int tl_engine_prefix_cache(tl_engine *e, int enabled, int max_retained_pages) {
    TL_REQUIRE(e, "engine_prefix_cache: null engine");
    TL_REQUIRE(enabled == 0 || enabled == 1, "engine_prefix_cache: enabled is 0 or 1");
    TL_REQUIRE(max_retained_pages >= 0, "engine_prefix_cache: max_retained_pages must be nonnegative (0 = no cap)");
    if (!enabled) {
        e->table.prefix_disable();
        return TL_OK;
    }
    TL_TRY(ensure_pool_table(e));
    e->table.prefix_enable(max_retained_pages);
    return TL_OK;
}

extern "C" int tl_engine_prefix_clear(tl_engine *e) {
    TL_REQUIRE(e, "engine_prefix_clear: null engine");
    e->table.pool.clear();
    return TL_OK;
}

extern "C" int tl_engine_prefix_stats(const tl_engine *e, tl_prefix_stats *out) {
    TL_REQUIRE(e && out, "engine_prefix_stats: null argument");
    const PagePool &pool = e->table.pool;
    const PrefixCounters &k = pool.ctr;
    *out = tl_prefix_stats{k.lookups, k.hits, k.tokens_matched, k.tail_rows_copied, k.pages_registered, k.pages_evicted,
                           pool.n_entries, pool.retained, pool.max_retained, pool.enabled ? 1 : 0};
    return TL_OK;
}

extern "C" int tl_engine_prefix_extend(tl_engine *e, int slot, const int32_t *tokens, int n) {
    TL_TRY(slot_check_unparked(e, slot));
    TL_REQUIRE(tokens && n >= 1, "engine_prefix_extend: need at least one token");
    if (!e->table.pool.enabled || e->lora_slot(slot)) return TL_OK;  // (a slot with a LoRA adapter bypasses the cache: nothing becomes known)
    for (int i = 0; i < n; ++i) TL_REQUIRE(tokens[i] >= 0 && tokens[i] < e->cfg.vocab_size, "engine_prefix_extend: token id out of range");
    return table_rc(e->table.extend(slot, tokens, n));
}

extern "C" int tl_engine_prefix_attach(tl_engine *e, int slot, const int32_t *tokens, int n, int *matched) {
    TL_TRY(slot_check_unparked(e, slot));
    TL_REQUIRE(tokens && matched && n >= 1, "engine_prefix_attach: need at least one token and a place for the result");
    const tl_engine_config &c = e->cfg;
    if (e->lora_slot(slot)) {  // K/V depend on the adapter and the index is keyed by token ids alone: a slot with an adapter matches nothing
        TL_REQUIRE(e->table.slots[slot].ctx == 0 && e->table.slots[slot].pages.empty(), "engine_prefix_attach: the slot already holds tokens or pages");
        *matched = 0;
        return TL_OK;
    }
    SlotEdits ed;
    TL_TRY(table_rc(e->table.attach(slot, tokens, n, ed, matched)));
    const int got = *matched;
    if (got == 0) return TL_OK;
    Pokes pk;
    TL_TRY(apply_edits(e, ed, pk));  // the tail rows' copy before the row and the context
    pk.emplace_back(e->context_lens + slot, got);
    TL_TRY(poke(e, pk));
    if (step_processes_slot(e, slot)) {  // the matched tokens are prompt tokens of the slot's history, as a prefill would have marked them
        for (int at = 0; at < got; at += c.max_prefill_rows) {
            const int len = std::min(c.max_prefill_rows, got - at);
            TL_HIP(hipMemcpyAsync(e->prefill_tokens, tokens + at, (size_t)len * 4, hipMemcpyHostToDevice, e->stream));
            const LogitMarkArgs mk{e->prefill_tokens, len, c.vocab_size, e->sdev<uint32_t>(SB_PROCESS, e->settings.at.pen_history), (long)slot * c.vocab_size};
            hipLaunchKernelGGL(logit_mark_prompt_kernel, dim3(ceil_div(len, 256)), dim3(256), 0, e->stream, mk);
            if (step_records_slot(e, slot)) launch_dry_record(e, slot, e->prefill_tokens, len, at);  // (the slot held no tokens: they start at 0)
            TL_CHECK_LAUNCH("engine prompt marking");
        }
    }
    if (e->settings.lookup_on(slot)) {  // ... and ids of the history of a slot armed for prompt lookup (lookup.h)
        for (int at = 0; at < got; at += c.max_prefill_rows) {
            const int len = std::min(c.max_prefill_rows, got - at);
            TL_HIP(hipMemcpyAsync(e->prefill_tokens, tokens + at, (size_t)len * 4, hipMemcpyHostToDevice, e->stream));
            TL_TRY(lookup_record_chunk(e, slot, e->prefill_tokens, len, at));
        }
    }
    return TL_OK;
}

// Move a (prefilled) sequence from slot `src` to the free slot `dst`: the reference prefills a request in its own
// cache and then adopts it into a batch slot (BatchingKvCache.add_request, kv_cache.py:226-238); here only the
// block-table row, context length and pending token change hands — no K/V byte moves.
extern "C" int tl_engine_move(tl_engine *e, int src, int dst) {
    TL_REQUIRE(e, "engine: null engine");
    TL_TRY(stop_reconcile(e));
    if (!e->table.check(src, true)) TL_TRY(lookup_catch_up(e, src));  // (as in tl_engine_fork)
    SlotEdits ed;
    Pokes pk;
    TL_TRY(table_rc(e->table.move(src, dst, ed)));
    TL_TRY(apply_edits(e, ed, pk));
    // a parked sequence stays parked at dst: no sequence on the device, its host records have moved with it
    const Slot &d = e->table.slots[dst];
    pk.emplace_back(e->context_lens + dst, d.parked ? 0 : d.ctx);
    pk.emplace_back(e->context_lens + src, 0);
    pk.emplace_back(e->live + dst, d.parked || d.stopped ? 0 : 1);  // (a stopped sequence stays stopped at dst)
    pk.emplace_back(e->live + src, 0);
    pk.emplace_back(e->produced + dst, 0);
    TL_TRY(settings_carry(e, src, dst, true, pk));
    return lookup_store_pending(e, dst);
}

// ---- beam search (include/tinyllm_engine.h "Beam search"; the selection is beam.h, the group's genealogy slot_table.h) ----------------
// Why the slot cannot be a beam, or null: a group decodes through the plain greedy program and selects from the raw rows
static const char *beam_slot_refusal(const tl_engine *e, int slot) {
    const Slot &s = e->table.slots[slot];
    if (!s.live) return "engine_beam: slot holds no sequence";
    if (s.parked) return "engine_beam: the slot is parked (tl_engine_unpark first)";
    if (s.stopped) return "engine_beam: the slot has stopped";
    return e->settings.refuses_beam(slot);
}

extern "C" int tl_engine_beam_select(tl_engine *e, int row0, int rows, const float *scores_host, int n_cand, tl_beam_candidate *out_host) {
    TL_REQUIRE(e && scores_host && out_host, "engine_beam_select: null argument");
    TL_REQUIRE(rows >= 1 && rows <= TL_MAX_BEAMS, "engine_beam_select: rows must be 1 .. 8");
    TL_REQUIRE(n_cand >= 1 && n_cand <= TL_MAX_BEAM_CANDIDATES, "engine_beam_select: n_cand must be 1 .. 32");
    TL_REQUIRE(e->cfg.vocab_size <= SMP_MAX_VOCAB, "engine_beam_select: vocabulary larger than the sampler's 524,288 tokens");
    TL_REQUIRE(e->logits_slot != -2, "engine_beam_select: the most recent logits are a packed prefill's");
    TL_REQUIRE(row0 >= 0 && row0 <= e->logits_rows - rows, "engine_beam_select: the rows are not inside the most recent logits");
    TL_TRY(stop_reconcile(e));
    for (int i = 0; i < rows; ++i) TL_TRY(table_rc(beam_slot_refusal(e, e->logits_slot >= 0 ? e->logits_slot : row0 + i)));
    if (!e->beam_mem) {
        Carve carve;
        const size_t scores = carve(TL_MAX_BEAMS * sizeof(float)), out = carve(TL_MAX_BEAM_CANDIDATES * sizeof(tl_beam_candidate)),
                     survivors = carve(BM_SURVIVORS * sizeof(tl_beam_candidate));
        TL_TRY(e->beam_mem.alloc(carve.off, "engine_beam_select: hipMalloc(scratch) failed"));
        e->beam_scores = e->beam_mem.at<float>(scores);
        e->beam_out = e->beam_mem.at<tl_beam_candidate>(out);
        e->beam_survivors = e->beam_mem.at<tl_beam_candidate>(survivors);
        e->stats.workspace_bytes += carve.off;
    }
    TL_HIP(hipMemcpyAsync(e->beam_scores, scores_host, (size_t)rows * sizeof(float), hipMemcpyHostToDevice, e->stream));
    TL_TRY(beam_rows_launch(e->logits + (size_t)row0 * e->cfg.vocab_size, rows, e->cfg.vocab_size, e->beam_scores, n_cand, e->beam_survivors,
                            e->beam_out, e->stream));
    TL_HIP(hipMemcpyAsync(out_host, e->beam_out, (size_t)n_cand * sizeof(tl_beam_candidate), hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    return TL_OK;
}

extern "C" int tl_engine_beam_reorder(tl_engine *e, int slot0, int n_src, int width, const int *parents, const int32_t *tokens) {
    TL_REQUIRE(e && parents && tokens, "engine_beam_reorder: null argument");
    TL_REQUIRE(n_src >= 1 && n_src <= TL_MAX_BEAMS && width >= 1 && width <= TL_MAX_BEAMS, "engine_beam_reorder: n_src and width are 1 .. 8");
    const int span = std::max(n_src, width);
    TL_REQUIRE(slot0 >= 0 && slot0 <= e->cfg.max_batch - span, "engine_beam_reorder: slots out of range");
    for (int i = 0; i < width; ++i) {
        TL_REQUIRE(parents[i] >= 0 && parents[i] < n_src, "engine_beam_reorder: parent out of range");
        TL_REQUIRE(tokens[i] >= 0 && tokens[i] < e->cfg.vocab_size, "engine_beam_reorder: token id out of range");
    }
    TL_TRY(stop_reconcile(e));
    for (int i = 0; i < n_src; ++i) TL_TRY(table_rc(beam_slot_refusal(e, slot0 + i)));
    TL_TRY(ensure_pool_table(e));  // (the tail copies' pool table: built by the first call that needs it, before anything changes)
    SlotEdits ed;
    Pokes pk;
    TL_TRY(table_rc(e->table.beam_reorder(slot0, n_src, width, parents, ed)));
    TL_TRY(apply_edits(e, ed, pk));  // the tail copies before the row entries that publish the fresh pages
    for (int i = 0; i < span; ++i) {
        const int slot = slot0 + i;
        const Slot &d = e->table.slots[slot];
        pk.emplace_back(e->live + slot, d.live ? 1 : 0);
        pk.emplace_back(e->context_lens + slot, d.ctx);
        pk.emplace_back(e->tokens + slot, i < width ? tokens[i] : 0);
        if (i < width) pk.emplace_back(e->produced + slot, 0);
    }
    SettingsEdits sed;
    e->settings.beam_reorder(slot0, n_src, width, parents, sed);  // the adapters and the pending flags follow the parents
    return settings_apply(e, sed, pk);
}


// ---- KV swap (include/tinyllm_engine.h "KV swap"; kernels kv_swap.h, host accounting slot_table.h) ------------------------------------
static int swap_free(tl_engine *e) {
    if (!e->swap_host && !e->swap_staging) return TL_OK;
    TL_HIP(hipStreamSynchronize(e->stream));  // copies into / out of the arena may be in flight
    e->swap_host.reset();
    e->swap_staging.reset();
    e->stats.workspace_bytes -= (size_t)e->swap_staging_pages * e->swap_record_bytes;
    e->swap_staging_pages = 0;
    e->table.arena.init(0);
    return TL_OK;
}

extern "C" int tl_engine_swap_space(tl_engine *e, int host_pages) {
    TL_REQUIRE(e, "engine_swap_space: null engine");
    TL_REQUIRE(host_pages >= 0, "engine_swap_space: host_pages must be nonnegative (0 frees the swap space)");
    for (const Slot &s : e->table.slots) TL_REQUIRE(!s.parked, "engine_swap_space: a slot is parked (unpark or release it first)");
    TL_TRY(swap_free(e));
    if (host_pages == 0) return TL_OK;
    const tl_engine_config &c = e->cfg;
    TL_TRY(ensure_pool_table(e));
    const size_t rec = kv_page_record_bytes(e->kv_pools_host.data(), e->kv_pools_n, c.num_kv_heads, c.page_size);
    if (!e->swap_offsets_dev) {
        std::vector<size_t> offsets(e->kv_pools_n);
        size_t at = 0;
        for (int i = 0; i < e->kv_pools_n; ++i) {
            offsets[i] = at;
            at += (size_t)c.num_kv_heads * c.page_size * e->kv_pools_host[i].row_bytes;
        }
        TL_TRY(alloc_filled(e->swap_offsets_mem, offsets.size() * sizeof(size_t), "engine_swap_space: hipMalloc(record offsets) failed", [&](char *m) -> int {
            const hipError_t rc = hipMemcpy(m, offsets.data(), offsets.size() * sizeof(size_t), hipMemcpyHostToDevice);
            return rc == hipSuccess ? TL_OK : fail(TL_ERR_HIP, std::string("engine_swap_space: hipMemcpy(record offsets): ") + hipGetErrorString(rc));
        }));
        e->swap_offsets_dev = e->swap_offsets_mem.at<size_t>();
    }
    // the staging buffer: up to 32 MiB of records (a group of pages per gather + copy), at least one, never more than the arena holds
    const int staging_pages = (int)std::min<size_t>((size_t)host_pages, std::max<size_t>(1, ((size_t)32 << 20) / rec));
    DeviceBlock host, staging;  // both, or the engine keeps neither
    TL_TRY(host.alloc_pinned((size_t)host_pages * rec, "engine_swap_space: hipHostMalloc(host arena) failed"));
    TL_TRY(staging.alloc((size_t)staging_pages * rec, "engine_swap_space: hipMalloc(staging) failed"));
    e->swap_host = std::move(host), e->swap_staging = std::move(staging);
    e->swap_record_bytes = rec;
    e->swap_staging_pages = staging_pages;
    e->table.arena.init(host_pages);
    e->stats.workspace_bytes += (size_t)staging_pages * rec;
    return TL_OK;
}

extern "C" int tl_engine_park(tl_engine *e, int slot) {
    TL_REQUIRE(e, "engine: null engine");
    TL_TRY(stop_reconcile(e));
    TL_TRY(table_rc(e->table.park_begin(slot)));
    const tl_engine_config &c = e->cfg;
    const Slot &s = e->table.slots[slot];
    const std::vector<int> &records = s.records;
    const int ctx = s.ctx, n = (int)records.size();
    // the pages leave through the slot's block-table row, which holds their ids on the device already; everything below is enqueued
    // before the row is cleared and before anybody can take a freed page
    const int32_t *row = e->block_table + (size_t)slot * c.max_pages_per_seq;
    const size_t rec = e->swap_record_bytes;
    int rc = TL_OK;
    for (int j0 = 0; j0 < n && rc == TL_OK; j0 += e->swap_staging_pages) {
        const int j1 = std::min(n, j0 + e->swap_staging_pages);
        const int tail = j1 == n ? ctx - (n - 1) * c.page_size : c.page_size;
        rc = kv_swap_pages<true>(e->kv_pools_dev, e->swap_offsets_dev, e->kv_pools_n, c.num_kv_heads, c.page_size, row + j0, j1 - j0, tail,
                                 e->swap_staging.at(), rec, e->stream);
        for (const auto &run : swap_runs(records, j0, j1)) {  // one copy per group while the arena hands out consecutive records
            if (rc != TL_OK) break;
            if (hipMemcpyAsync(e->swap_host.at((size_t)records[run.first] * rec), e->swap_staging.at((size_t)(run.first - j0) * rec),
                               (size_t)run.second * rec, hipMemcpyDeviceToHost, e->stream) != hipSuccess)
                rc = fail(TL_ERR_HIP, "engine_park: hipMemcpyAsync(device to host) failed");
        }
    }
    if (rc != TL_OK) {  // nothing of the slot has changed: the records go back
        e->table.park_abort(slot);
        return rc;
    }
    SlotEdits ed;
    Pokes pk;
    e->table.park_commit(slot, ed);
    TL_TRY(apply_edits(e, ed, pk));
    pk.emplace_back(e->live + slot, 0);
    pk.emplace_back(e->context_lens + slot, 0);
    e->swap_parks++;
    e->swap_pages_out += n;
    SettingsEdits sed;
    e->settings.park(slot, sed);  // (the processing parameters go neutral on the device)
    return settings_apply(e, sed, pk);
}

extern "C" int tl_engine_unpark(tl_engine *e, int slot) {
    TL_REQUIRE(e, "engine: null engine");
    const tl_engine_config &c = e->cfg;
    SlotEdits ed;
    Pokes pk;
    std::vector<int> records;
    TL_TRY(table_rc(e->table.unpark(slot, ed, records)));
    const int ctx = e->table.slots[slot].ctx, n = (int)records.size();
    e->swap_unparks++;
    e->swap_pages_in += n;
    TL_TRY(apply_edits(e, ed, pk));
    TL_TRY(poke(e, pk));  // the row first: the scatter reads the page ids from it
    const int32_t *row = e->block_table + (size_t)slot * c.max_pages_per_seq;
    const size_t rec = e->swap_record_bytes;
    for (int j0 = 0; j0 < n; j0 += e->swap_staging_pages) {
        const int j1 = std::min(n, j0 + e->swap_staging_pages);
        const int tail = j1 == n ? ctx - (n - 1) * c.page_size : c.page_size;
        for (const auto &run : swap_runs(records, j0, j1))
            TL_HIP(hipMemcpyAsync(e->swap_staging.at((size_t)(run.first - j0) * rec), e->swap_host.at((size_t)records[run.first] * rec),
                                  (size_t)run.second * rec, hipMemcpyHostToDevice, e->stream));
        TL_TRY(kv_swap_pages<false>(e->kv_pools_dev, e->swap_offsets_dev, e->kv_pools_n, c.num_kv_heads, c.page_size, row + j0, j1 - j0, tail,
                                    e->swap_staging.at(), rec, e->stream));
    }
    pk.emplace_back(e->context_lens + slot, ctx);
    pk.emplace_back(e->live + slot, e->table.slots[slot].stopped ? 0 : 1);  // (an unparked stopped slot stays stopped)
    SettingsEdits sed;
    e->settings.unpark(slot, sed);  // (... and come back from the mirror)
    return settings_apply(e, sed, pk);
}

extern "C" int tl_engine_slot_parked(const tl_engine *e, int slot) {
    if (!e || e->table.check(slot, true)) return -1;
    return e->table.slots[slot].parked ? 1 : 0;
}

extern "C" int tl_engine_step_pages(const tl_engine *e, int batch, int *need, int *obtainable) {
    TL_REQUIRE(e && need && obtainable, "engine_step_pages: null argument");
    TL_REQUIRE(batch > 0 && batch <= e->cfg.max_batch, "engine_step_pages: batch out of range");
    int extra = 0;
    for (int b = 0; b < batch; ++b) {
        if (!e->slot_runs(b)) continue;
        const Slot &s = e->table.slots[b];
        extra += std::max(0, swap_pages_of(s.ctx + 1, e->cfg.page_size) - (int)s.pages.size());
    }
    *need = extra;
    *obtainable = (int)e->table.pool.available();
    return TL_OK;
}

extern "C" int tl_engine_swap_stats(const tl_engine *e, tl_swap_stats *out) {
    TL_REQUIRE(e && out, "engine_swap_stats: null argument");
    *out = tl_swap_stats{e->table.arena.capacity(), e->table.arena.in_use, e->swap_parks, e->swap_unparks, e->swap_pages_out, e->swap_pages_in,
                         e->swap_host ? e->swap_record_bytes : 0};
    return TL_OK;
}

// Pending token ids of slots [0, count) after synchronising the stream (one copy per decode step instead of one
// ring read per slot).
extern "C" int tl_engine_read_pending(tl_engine *e, int count, int32_t *out) {
    TL_REQUIRE(e && out, "engine_read_pending: null argument");
    TL_REQUIRE(count > 0 && count <= e->cfg.max_batch, "engine_read_pending: count out of range");
    TL_HIP(hipStreamSynchronize(e->stream));
    TL_HIP(hipMemcpy(out, e->tokens, (size_t)count * 4, hipMemcpyDeviceToHost));
    return TL_OK;
}

extern "C" int tl_engine_context_len(const tl_engine *e, int slot) {
    if (!e || e->table.check(slot, true)) return -1;
    return e->table.slots[slot].ctx;
}

extern "C" int tl_engine_set_token(tl_engine *e, int slot, int32_t token) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(token >= 0 && token < e->cfg.vocab_size, "engine_set_token: token id out of range");
    TL_TRY(table_rc(e->settings.refuses_set_token(slot)));
    Pokes pk;
    pk.emplace_back(e->tokens + slot, token);
    TL_TRY(poke(e, pk));
    return lookup_store_pending(e, slot);  // (an armed slot: the ring will not hold this token)
}

extern "C" int tl_engine_set_sampling(tl_engine *e, int slot, float temperature, int top_k, float top_p, uint64_t seed) {
    TL_TRY(slot_check(e, slot, true));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_sampling(slot, temperature, top_k, top_p, seed, ed); });
}

extern "C" int tl_engine_set_truncation(tl_engine *e, int slot, float min_p, float typical_p) {
    TL_TRY(slot_check(e, slot, true));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_truncation(slot, min_p, typical_p, ed); });
}

extern "C" int tl_engine_set_mirostat(tl_engine *e, int slot, float tau, float eta) {
    TL_TRY(slot_check(e, slot, true));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_mirostat(slot, tau, eta, ed); });
}

extern "C" int tl_engine_mirostat_mu(tl_engine *e, int slot, float *mu) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(mu, "engine_mirostat_mu: null argument");
    *mu = __builtin_nanf("");
    if (!e->settings_mem[SB_TRUNC]) return TL_OK;
    TL_HIP(hipStreamSynchronize(e->stream));
    TL_HIP(hipMemcpy(mu, e->sdev<float>(SB_TRUNC, e->settings.at.trn_mu) + slot, sizeof(float), hipMemcpyDeviceToHost));
    return TL_OK;
}

extern "C" int tl_engine_copy_filtered_logits(tl_engine *e, void *dst_dev, int rows) {
    TL_REQUIRE(e && dst_dev, "engine_copy_filtered_logits: null argument");
    TL_REQUIRE(rows > 0 && rows <= e->cfg.max_batch, "engine_copy_filtered_logits: rows out of range");
    TL_REQUIRE(e->settings_mem[SB_TRUNC], "engine_copy_filtered_logits: no slot of this engine has truncated yet");
    TL_HIP(hipMemcpyAsync(dst_dev, e->sdev<uint16_t>(SB_TRUNC, e->settings.at.trn_rows), (size_t)rows * e->cfg.vocab_size * 2, hipMemcpyDeviceToDevice, e->stream));
    return TL_OK;
}

extern "C" int tl_truncate_rows(const void *logits_dev, int rows, int vocab, const float *temperature_dev, const float *min_p_dev, const float *typical_p_dev,
                                const float *mu_dev, void *out_dev, float *kept_logsum_dev, void *stream) {
    TL_REQUIRE(logits_dev && temperature_dev && min_p_dev && typical_p_dev && mu_dev && out_dev, "truncate_rows: null argument");
    TL_REQUIRE(logits_dev != out_dev, "truncate_rows: rows are never filtered in place");
    TL_REQUIRE(rows > 0 && rows <= 65535, "truncate_rows: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "truncate_rows: vocabulary out of range (1 .. 524,288)");
    const TruncateArgs a{(const uint16_t *)logits_dev, (uint16_t *)out_dev, vocab, 0, temperature_dev, min_p_dev, typical_p_dev, mu_dev, kept_logsum_dev, nullptr};
    hipLaunchKernelGGL(truncate_rows_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("truncate_rows");
    return TL_OK;
}

extern "C" int tl_mirostat_update_rows(const void *filtered_dev, int rows, int vocab, const int32_t *ids_dev, const float *temperature_dev,
                                       const float *kept_logsum_dev, const float *tau_dev, const float *eta_dev, float *mu_dev, void *stream) {
    TL_REQUIRE(filtered_dev && ids_dev && temperature_dev && kept_logsum_dev && tau_dev && eta_dev && mu_dev, "mirostat_update_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "mirostat_update_rows: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "mirostat_update_rows: vocabulary out of range (1 .. 524,288)");
    const MirostatUpdateArgs a{(const uint16_t *)filtered_dev, vocab, 0, ids_dev, temperature_dev, kept_logsum_dev, tau_dev, eta_dev, mu_dev, nullptr, nullptr};
    hipLaunchKernelGGL(mirostat_update_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("mirostat_update_rows");
    return TL_OK;
}

extern "C" int tl_engine_set_penalties(tl_engine *e, int slot, float repetition_penalty, float presence_penalty, float frequency_penalty) {
    TL_TRY(slot_check(e, slot, true));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_penalties(slot, repetition_penalty, presence_penalty, frequency_penalty, ed); });
}

extern "C" int tl_engine_set_dry(tl_engine *e, int slot, float multiplier, float base, int allowed_length, int range, int no_repeat_ngram,
                                 const int32_t *breaker_ids, int n_breakers) {
    TL_TRY(slot_check(e, slot, true));
    TL_TRY(stop_reconcile(e));  // (the context length of a slot a stop froze in mid-call)
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) {
        return e->settings.set_dry(slot, multiplier, base, allowed_length, range, no_repeat_ngram, breaker_ids, n_breakers, e->table.slots[slot].ctx, ed);
    });
}

extern "C" int tl_dry_rows(int32_t *sequences_dev, int rows, int cap, const int32_t *start_dev, const int32_t *end_dev, const float *multiplier_dev,
                           const float *base_dev, const int32_t *allowed_length_dev, const int32_t *range_dev, const int32_t *no_repeat_ngram_dev,
                           const int32_t *breaker_ids_dev, const int32_t *n_breakers_dev, uint32_t *table_dev, void *logits_dev, int vocab, void *stream) {
    TL_REQUIRE(sequences_dev && start_dev && end_dev && multiplier_dev && base_dev && allowed_length_dev && range_dev && no_repeat_ngram_dev &&
                   n_breakers_dev && table_dev && logits_dev, "dry_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "dry_rows: rows out of range");
    TL_REQUIRE(cap > 0, "dry_rows: sequence capacity out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "dry_rows: vocabulary out of range (1 .. 524,288)");
    // (without breaker lists every count must be 0: the kernel reads no entry then)
    DryArgs a{};
    a.seq = sequences_dev, a.table = table_dev, a.rows = (uint16_t *)logits_dev, a.cap = cap, a.vocab = vocab, a.pos = end_dev;
    a.multiplier = multiplier_dev, a.base = base_dev, a.allowed = allowed_length_dev, a.range = range_dev, a.ngram = no_repeat_ngram_dev;
    a.start = start_dev, a.n_breakers = n_breakers_dev, a.breakers = breaker_ids_dev;
    hipLaunchKernelGGL(dry_match_kernel, dim3(rows), dim3(DRY_MATCH_THREADS), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(dry_apply_kernel, dim3(ceil_div(vocab, DRY_APPLY_CHUNK), rows), dim3(DRY_APPLY_THREADS), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("dry_rows");
    return TL_OK;
}

// ---- prompt lookup (include/tinyllm_engine.h "Prompt lookup"; the kernels are lookup.h, the accounting slot_settings.h) -------------------
static int lookup_params_check(const char *who, int max_ngram, int min_ngram, int num_proposals) {
    const std::string w = std::string(who) + ": ";
    TL_REQUIRE(max_ngram >= 1 && max_ngram <= LOOKUP_MAX_NGRAM, w + "max_ngram must be 1 .. 16");
    TL_REQUIRE(min_ngram >= 1 && min_ngram <= max_ngram, w + "min_ngram must be 1 .. max_ngram");
    TL_REQUIRE(num_proposals >= 1 && num_proposals <= LOOKUP_MAX_PROPOSALS, w + "num_proposals must be 1 .. 7");
    return TL_OK;
}

extern "C" int tl_lookup_rows(const int32_t *sequences_dev, int rows, int cap, const int32_t *start_dev, const int32_t *end_dev, int max_ngram, int min_ngram,
                              int num_proposals, int32_t *proposals_dev, int32_t *counts_dev, int32_t *match_dev, void *stream) {
    TL_REQUIRE(sequences_dev && start_dev && end_dev && proposals_dev && counts_dev, "lookup_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "lookup_rows: rows out of range");
    TL_REQUIRE(cap > 0 && cap <= (1 << LOOKUP_POS_BITS), "lookup_rows: sequence capacity out of range (1 .. 16,777,216)");
    TL_TRY(lookup_params_check("lookup_rows", max_ngram, min_ngram, num_proposals));
    LookupArgs a{};
    a.seq = const_cast<int32_t *>(sequences_dev), a.cap = cap, a.start = start_dev, a.end = end_dev;  // (this launch stores nothing to the rows)
    a.max_ngram = max_ngram, a.min_ngram = min_ngram, a.k = num_proposals;
    a.proposals = proposals_dev, a.counts = counts_dev, a.match = match_dev;
    hipLaunchKernelGGL(lookup_rows_kernel, dim3(rows), dim3(LOOKUP_THREADS), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("lookup_rows");
    return TL_OK;
}

extern "C" int tl_engine_set_lookup(tl_engine *e, int slot, int on) {
    TL_TRY(slot_check(e, slot, true));
    TL_TRY(stop_reconcile(e));  // (the context length of a slot a stop froze in mid-call)
    const bool was = e->settings.lookup_on(slot);
    Pokes pk;
    TL_TRY(settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_lookup(slot, on != 0, e->table.slots[slot].ctx, ed); }));
    return on && !was ? lookup_store_pending(e, slot) : (int)TL_OK;  // (whatever pending token the slot holds: the ring may not know it)
}

extern "C" int tl_engine_lookup_state(const tl_engine *e, int slot, int *armed, int *start, int *recorded) {
    TL_TRY(slot_check(e, slot, false));
    const SlotSettings::State &s = e->settings.slots[slot];
    if (armed) *armed = s.lookup ? 1 : 0;
    if (start) *start = s.lk_s0;
    if (recorded) *recorded = s.lk_rec;
    return TL_OK;
}

// the body of tl_engine_lookup_propose and tl_engine_lookup_propose_sampled (sampled: the slots are those tl_engine_verify_batch_sampled takes)
static int lookup_propose_call(tl_engine *e, int n_seqs, const int *slots, const int *max_lens, int max_ngram, int min_ngram, int num_proposals,
                               int32_t *tokens_out, int *lens_out, bool sampled) {
    TL_REQUIRE(e && slots && tokens_out && lens_out, "engine_lookup_propose: null argument");
    TL_REQUIRE(n_seqs >= 1 && n_seqs <= LOOKUP_MAX_SLOTS, "engine_lookup_propose: between 1 and 64 sequences per call");
    TL_TRY(lookup_params_check("engine_lookup_propose", max_ngram, min_ngram, num_proposals));
    TL_TRY(stop_reconcile(e));
    LookupSlots rows{};
    int total = 0;
    for (int i = 0; i < n_seqs; ++i) {
        TL_TRY(slot_check_feeds(e, slots[i]));  // what tl_engine_verify_batch refuses: parked, stopped, ...
        TL_TRY(table_rc(sampled ? e->settings.refuses_verify_batch_sampled(slots[i]) : e->settings.refuses_verify_batch(slots[i])));
        TL_REQUIRE(e->settings.lookup_on(slots[i]), "engine_lookup_propose: a slot is not armed (tl_engine_set_lookup)");
        for (int j = 0; j < i; ++j) TL_REQUIRE(slots[j] != slots[i], "engine_lookup_propose: a slot appears twice");
        const int max_len = max_lens ? max_lens[i] : VERIFY_MAX_LEN;
        TL_REQUIRE(max_len >= 1 && max_len <= VERIFY_MAX_LEN, "engine_lookup_propose: max_lens must be 1 .. 8");
        total += max_len;
        const Slot &t = e->table.slots[slots[i]];
        const SlotSettings::State &s = e->settings.slots[slots[i]];
        rows.s[i] = {slots[i], s.lk_s0, s.lk_rec, t.ctx, t.produced, std::min(num_proposals, max_len - 1)};
    }
    TL_REQUIRE(total <= VERIFY_BATCH_ROWS, "engine_lookup_propose: the chunks together may exceed 64 rows (the sum of max_lens)");
    TL_TRY(aql_drain(e));  // (steps of the AQL route wrote the ring)
    int32_t *out = e->sdev<int32_t>(SB_LOOKUP, e->settings.at.lk_out);
    LookupArgs a{};
    a.seq = e->sdev<int32_t>(SB_LOOKUP, e->settings.at.lk_seq), a.cap = e->settings.sz.lookup_seq_cap;
    a.max_ngram = max_ngram, a.min_ngram = min_ngram, a.k = num_proposals;
    a.proposals = out, a.counts = out + LOOKUP_MAX_SLOTS * LOOKUP_ROW;
    const LookupRing r{e->ring, e->tokens, e->ring_cap};
    hipLaunchKernelGGL(lookup_engine_kernel, dim3(n_seqs), dim3(LOOKUP_THREADS), 0, e->stream, a, r, rows);
    TL_CHECK_LAUNCH("engine_lookup_propose");
    for (int i = 0; i < n_seqs; ++i) e->settings.lookup_caught_up(slots[i], rows.s[i].ctx);  // (the launch fetched what the ring held)
    int32_t host[LOOKUP_OUT_WORDS];
    TL_HIP(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    int at = 0;
    for (int i = 0; i < n_seqs; ++i) {
        const int n = std::min(std::max(host[LOOKUP_MAX_SLOTS * LOOKUP_ROW + i], 0), rows.s[i].k);
        lens_out[i] = 1 + n;
        for (int j = 0; j <= n; ++j) tokens_out[at++] = host[i * LOOKUP_ROW + j];
    }
    return TL_OK;
}

extern "C" int tl_engine_lookup_propose(tl_engine *e, int n_seqs, const int *slots, const int *max_lens, int max_ngram, int min_ngram, int num_proposals,
                                        int32_t *tokens_out, int *lens_out) {
    return lookup_propose_call(e, n_seqs, slots, max_lens, max_ngram, min_ngram, num_proposals, tokens_out, lens_out, false);
}

extern "C" int tl_engine_lookup_propose_sampled(tl_engine *e, int n_seqs, const int *slots, const int *max_lens, int max_ngram, int min_ngram,
                                                int num_proposals, int32_t *tokens_out, int *lens_out) {
    return lookup_propose_call(e, n_seqs, slots, max_lens, max_ngram, min_ngram, num_proposals, tokens_out, lens_out, true);
}

extern "C" int tl_engine_set_logit_bias(tl_engine *e, int slot, const int32_t *ids, const float *values, int n) {
    TL_TRY(slot_check(e, slot, true));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_logit_bias(slot, ids, values, n, ed); });
}

// ---- grammars (grammar.h) ----------------------------------------------------------------------------------------------------------
extern "C" int tl_vocab_create(int vocab, const int32_t *offsets, const uint8_t *bytes, void *stream, tl_vocab **out) {
    TL_REQUIRE(out, "vocab_create: null argument");
    *out = nullptr;
    TL_REQUIRE(offsets, "vocab_create: null argument");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "vocab_create: vocabulary out of range (1 .. 524,288)");
    TL_REQUIRE(offsets[0] == 0, "vocab_create: offsets[0] must be 0");
    for (int j = 0; j < vocab; ++j) TL_REQUIRE(offsets[j + 1] >= offsets[j], "vocab_create: offsets must be non-decreasing");
    const size_t nb = (size_t)offsets[vocab];
    TL_REQUIRE(nb == 0 || bytes, "vocab_create: null bytes");
    auto v = std::make_unique<tl_vocab>();
    v->vocab = vocab;
    v->offsets.assign(offsets, offsets + vocab + 1);
    v->bytes.assign(bytes, bytes + nb);
    std::vector<int32_t> long_index((size_t)vocab, 0);
    for (int j = 0; j < vocab; ++j)
        if (offsets[j + 1] - offsets[j] > GR_LONG) {
            long_index[j] = (int32_t)v->long_ids.size();
            v->long_ids.push_back(j);
        }
    const size_t o_bytes = align_up((size_t)(vocab + 1) * 4, 256), o_index = o_bytes + align_up(nb + 16, 256),
                 o_ids = o_index + align_up((size_t)vocab * 4, 256), total = o_ids + align_up(v->long_ids.size() * 4 + 4, 256);
    TL_TRY(v->mem.alloc(total, "vocab_create: hipMalloc failed"));
    v->offsets_dev = v->mem.at<int32_t>(), v->bytes_dev = v->mem.at<uint8_t>(o_bytes);
    v->long_index_dev = v->mem.at<int32_t>(o_index), v->long_ids_dev = v->mem.at<int32_t>(o_ids);
    hipError_t he = hipMemcpyAsync(v->offsets_dev, v->offsets.data(), (size_t)(vocab + 1) * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he == hipSuccess && nb) he = hipMemcpyAsync(v->bytes_dev, v->bytes.data(), nb, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he == hipSuccess) he = hipMemcpyAsync(v->long_index_dev, long_index.data(), (size_t)vocab * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he == hipSuccess && !v->long_ids.empty())
        he = hipMemcpyAsync(v->long_ids_dev, v->long_ids.data(), v->long_ids.size() * 4, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (he == hipSuccess) he = hipStreamSynchronize((hipStream_t)stream);
    if (he != hipSuccess) return fail(TL_ERR_HIP, std::string("vocab_create: ") + hipGetErrorString(he));
    *out = v.release();
    return TL_OK;
}

extern "C" void tl_vocab_destroy(tl_vocab *v) {
    delete v;
}

// tl_grammar_create (stack = false: ops, n_pop and pop_table unused) and tl_grammar_create_stack: validation, the host object, the device
// allocation headed by its GrammarDev, the uploads and the walks of the long tokens.  `who` heads every error text.
static int grammar_build(const std::string &who, bool stack, const tl_vocab *v, int n_states, const uint16_t *table, const uint8_t *ops, int n_pop,
                         const uint16_t *pop_table, const uint8_t *accepting, int start, const int32_t *eos_ids, int n_eos, void *stream, tl_grammar **out) {
    TL_REQUIRE(out, who + ": null argument");
    *out = nullptr;
    TL_REQUIRE(v && table && (ops || !stack) && accepting && eos_ids, who + ": null argument");
    TL_REQUIRE(n_states >= 1 && n_states <= GR_MAX_STATES, who + ": between 1 and 32,768 states");
    if (stack) TL_REQUIRE(n_pop >= 0 && n_pop <= GRS_MAX_POPS && (n_pop == 0 || pop_table), who + ": between 0 and 65,535 pop entries");
    TL_REQUIRE(start >= 0 && start < n_states, who + ": start state out of range");
    TL_REQUIRE(n_eos >= 1 && n_eos <= GR_MAX_EOS, who + ": between 1 and 8 EOS ids");
    for (int i = 0; i < n_eos; ++i) {
        TL_REQUIRE(eos_ids[i] >= 0 && eos_ids[i] < v->vocab, who + ": EOS id out of range");
        for (int k = 0; k < i; ++k) TL_REQUIRE(eos_ids[k] != eos_ids[i], who + ": an EOS id appears twice");
    }
    const size_t cells = (size_t)n_states * 256;
    auto g = std::make_unique<tl_grammar>();
    g->vocab = v, g->n_states = n_states, g->start = start, g->stack = stack, g->n_pop = stack ? n_pop : 0;
    if (!stack) {
        for (size_t i = 0; i < cells; ++i) TL_REQUIRE(table[i] == GR_DEAD || table[i] < n_states, who + ": a transition leads outside the table");
        g->table.assign(table, table + cells);
    } else {
        g->fused.resize(cells);
        for (size_t i = 0; i < cells; ++i) {
            TL_REQUIRE(ops[i] <= GRS_POP, who + ": an op byte is not 0 .. 5");
            if (table[i] != GR_DEAD) {
                if (ops[i] == GRS_POP) TL_REQUIRE(table[i] < n_pop, who + ": a pop entry leads outside the pop table");
                else TL_REQUIRE(table[i] < n_states, who + ": a transition leads outside the table");
            }
            g->fused[i] = (uint32_t)table[i] | (table[i] != GR_DEAD ? (uint32_t)ops[i] << 16 : 0u);
        }
        g->pop8.assign((size_t)std::max(n_pop, 1) * 8, (uint16_t)GR_DEAD);
        for (size_t i = 0; i < (size_t)n_pop * 5; ++i) {
            TL_REQUIRE(pop_table[i] == GR_DEAD || pop_table[i] < n_states, who + ": a pop leads outside the table");
            g->pop8[i / 5 * 8 + i % 5] = pop_table[i];
        }
    }
    g->accepting.assign(accepting, accepting + n_states);
    g->eos.assign(eos_ids, eos_ids + n_eos);
    // per (state, long token of the vocabulary): one bit, in rows of whole 64-bit ballots (long_bits), or one depth byte (long_m)
    const int n_long = (int)v->long_ids.size(), long_words = 2 * ceil_div(n_long, 64);
    const void *const table_host = stack ? (const void *)g->fused.data() : (const void *)g->table.data();
    const size_t table_bytes = cells * (stack ? 4 : 2), pop_bytes = g->pop8.size() * 2;
    Carve carve;
    static_assert(sizeof(GrammarDev) <= 256, "GrammarDev heads the grammar's allocation");
    carve(sizeof(GrammarDev));
    const size_t o_table = carve(table_bytes), o_pop = stack ? carve(pop_bytes) : 0, o_acc = carve((size_t)n_states),
                 o_long = carve(stack ? (size_t)n_states * n_long + 4 : (size_t)n_states * long_words * 4 + 4);
    TL_TRY(g->mem.alloc(carve.off, who + ": hipMalloc failed"));
    char *const mem = g->mem.at();
    GrammarDev d{};
    d.accepting = (const uint8_t *)(mem + o_acc);
    d.offsets = v->offsets_dev, d.bytes = v->bytes_dev, d.n_states = n_states, d.n_eos = n_eos, d.long_index = v->long_index_dev;
    for (int i = 0; i < GR_MAX_EOS; ++i) d.eos[i] = i < n_eos ? eos_ids[i] : -1;
    if (stack) {
        d.kind = 1, d.n_pop = n_pop, d.n_long = n_long;
        d.fused = (const uint32_t *)(mem + o_table), d.pop = (const uint16_t *)(mem + o_pop), d.long_m = (const uint8_t *)(mem + o_long);
    } else {
        d.table = (const uint16_t *)(mem + o_table), d.long_bits = (const uint32_t *)(mem + o_long), d.long_words = long_words;
    }
    const hipStream_t st = (hipStream_t)stream;
    hipError_t he = hipMemcpyAsync(mem, &d, sizeof(d), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(mem + o_table, table_host, table_bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && stack) he = hipMemcpyAsync(mem + o_pop, g->pop8.data(), pop_bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(mem + o_acc, g->accepting.data(), (size_t)n_states, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && n_long > 0) {  // the walks of the long tokens from every state (a stack grammar: with an empty stack), once, on the device
        if (stack) {
            const GrammarLongDepthArgs la{d.fused, d.pop, d.offsets, d.bytes, v->long_ids_dev, n_long, (uint8_t *)(mem + o_long)};
            hipLaunchKernelGGL(grammar_long_depth_kernel, dim3(ceil_div(n_long, 64), n_states), dim3(64), 0, st, la);
        } else {
            const GrammarLongArgs la{d.table, d.offsets, d.bytes, v->long_ids_dev, n_long, long_words, (uint32_t *)(mem + o_long)};
            hipLaunchKernelGGL(grammar_long_bits_kernel, dim3(long_words / 2, n_states), dim3(64), 0, st, la);
        }
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipStreamSynchronize(st);  // (the copies read this frame's `d`)
    if (he != hipSuccess) return fail(TL_ERR_HIP, who + ": " + hipGetErrorString(he));
    g->dev = (GrammarDev *)mem;
    *out = g.release();
    return TL_OK;
}

extern "C" int tl_grammar_create(const tl_vocab *v, int n_states, const uint16_t *table, const uint8_t *accepting, int start, const int32_t *eos_ids,
                                 int n_eos, void *stream, tl_grammar **out) {
    return grammar_build("grammar_create", false, v, n_states, table, nullptr, 0, nullptr, accepting, start, eos_ids, n_eos, stream, out);
}

extern "C" int tl_grammar_create_stack(const tl_vocab *v, int n_states, const uint16_t *table, const uint8_t *ops, int n_pop, const uint16_t *pop_table,
                                       const uint8_t *accepting, int start, const int32_t *eos_ids, int n_eos, void *stream, tl_grammar **out) {
    return grammar_build("grammar_create_stack", true, v, n_states, table, ops, n_pop, pop_table, accepting, start, eos_ids, n_eos, stream, out);
}

extern "C" void tl_grammar_destroy(tl_grammar *g) {
    delete g;
}

extern "C" int tl_engine_set_grammar(tl_engine *e, int slot, const tl_grammar *g) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(!g || g->vocab->vocab == e->cfg.vocab_size, "engine_set_grammar: the grammar's vocabulary is not the engine's size");
    const GrammarRef ref = g ? GrammarRef{(uint64_t)(uintptr_t)g->dev, g->stack, g->start, g} : GrammarRef{};
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_grammar(slot, ref, ed); });
}

// the configuration of a slot with grammar `g` (a regex grammar's: (state, 0, 0)) once everything submitted has run: the slot's record,
// advanced on the host with the pending token where no step has consumed that yet
static int gr_read_config(tl_engine *e, int slot, const tl_grammar *g, GrsConfig *out) {
    TL_HIP(hipStreamSynchronize(e->stream));
    GrsConfig c{GR_END, 0, 0ull};
    if (g->stack) {
        GrammarStackRecord rec{};
        TL_HIP(hipMemcpy(&rec, e->sdev<GrammarStackRecord>(SB_STACK, 0) + slot, sizeof(rec), hipMemcpyDeviceToHost));
        int which;
        c = grs_unpack((uint32_t)(rec.rec >> 32), &which);
        if (c.state >= 0) c.stack = rec.stack[which] & grs_mask(c.depth);
    } else {
        GrammarRecord rec{};
        TL_HIP(hipMemcpy(&rec, e->sdev<GrammarRecord>(SB_GRAMMAR, e->settings.at.gr_state) + slot, sizeof(rec), hipMemcpyDeviceToHost));
        c.state = rec.state;
    }
    int32_t pending = 0;
    TL_HIP(hipMemcpy(&pending, e->tokens + slot, 4, hipMemcpyDeviceToHost));
    *out = e->settings.slots[slot].gr_pending ? g->advance(c, pending) : c;
    return TL_OK;
}

extern "C" int tl_engine_grammar_state(tl_engine *e, int slot, int *state, int *accepting) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(state, "engine_grammar_state: null argument");
    const tl_grammar *g = e->grammar_of(slot);
    TL_REQUIRE(g, "engine_grammar_state: the slot has no grammar");
    GrsConfig c;
    TL_TRY(gr_read_config(e, slot, g, &c));
    *state = c.state;
    if (accepting) *accepting = c.state < 0 || g->accepting[c.state] ? 1 : 0;
    return TL_OK;
}

extern "C" int tl_engine_grammar_config(tl_engine *e, int slot, int *state, int *depth, uint64_t *stack, int *accepting) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(state && depth && stack, "engine_grammar_config: null argument");
    const tl_grammar *g = e->grammar_of(slot);
    TL_REQUIRE(g, "engine_grammar_config: the slot has no grammar");
    GrsConfig c;
    TL_TRY(gr_read_config(e, slot, g, &c));
    *state = c.state, *depth = c.depth, *stack = c.stack;
    if (accepting) *accepting = c.state < 0 || g->accepting[c.state] ? 1 : 0;
    return TL_OK;
}

// ---- stop conditions (include/tinyllm_engine.h "Stop conditions"; the automaton is stop_set.h, the launch stop.h) ---------------------
extern "C" int tl_stop_create(const tl_vocab *v, const int32_t *ids, int n_ids, const uint8_t *bytes, const int32_t *offsets, int n_strings,
                              void *stream, tl_stop **out) {
    TL_REQUIRE(out, "stop_create: null argument");
    *out = nullptr;
    TL_REQUIRE(n_strings <= 0 || v, "stop_create: stop strings need a vocabulary (tl_vocab_create)");
    auto s = std::make_unique<tl_stop>();
    if (const char *why = stop_set_build(v ? v->vocab : 0, ids, n_ids, bytes, offsets, n_strings, s->set)) return fail(TL_ERR_INVALID, why);
    const StopSet &h = s->set;
    s->vocab = v;
    Carve carve;
    const size_t o_dev = carve(sizeof(StopDev)), o_ids = carve(h.ids.size() * 4 + 4), o_table = carve(h.table.size() * 2 + 2),
                 o_match = carve(h.match.size() * 2 + 2), o_len = carve(h.match_len.size() * 2 + 2);
    TL_TRY(s->mem.alloc(carve.off, "stop_create: hipMalloc failed"));
    char *const mem = s->mem.at();
    StopDev d{};
    d.ids = (const int32_t *)(mem + o_ids);
    d.n_ids = (int)h.ids.size(), d.max_len = h.max_len, d.n_states = h.n_states;
    if (h.n_strings) {
        d.table = (const uint16_t *)(mem + o_table), d.match = (const int16_t *)(mem + o_match), d.match_len = (const uint16_t *)(mem + o_len);
    }
    if (v) d.offsets = v->offsets_dev, d.bytes = v->bytes_dev, d.vocab = v->vocab;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t he = hipMemcpyAsync(mem + o_dev, &d, sizeof(d), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && !h.ids.empty()) he = hipMemcpyAsync(mem + o_ids, h.ids.data(), h.ids.size() * 4, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && h.n_strings) he = hipMemcpyAsync(mem + o_table, h.table.data(), h.table.size() * 2, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && h.n_strings) he = hipMemcpyAsync(mem + o_match, h.match.data(), h.match.size() * 2, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && h.n_strings) he = hipMemcpyAsync(mem + o_len, h.match_len.data(), h.match_len.size() * 2, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);  // (the copies read this frame's `d`)
    if (he != hipSuccess) return fail(TL_ERR_HIP, std::string("stop_create: ") + hipGetErrorString(he));
    s->dev = (StopDev *)(mem + o_dev);
    *out = s.release();
    return TL_OK;
}

extern "C" void tl_stop_destroy(tl_stop *s) {
    delete s;
}

extern "C" int tl_engine_set_stop(tl_engine *e, int slot, const tl_stop *set, int max_new_tokens) {
    TL_TRY(slot_check(e, slot, true));
    // (the record refuses a negative budget too; here it keeps its place ahead of the set's checks, which need the tl_stop)
    TL_REQUIRE(max_new_tokens >= 0, "engine_set_stop: max_new_tokens must be nonnegative (0 = no budget)");
    if (set) {
        TL_REQUIRE(!set->vocab || set->vocab->vocab == e->cfg.vocab_size, "engine_set_stop: the set's vocabulary is not the engine's size");
        for (int32_t id : set->set.ids) TL_REQUIRE(id < e->cfg.vocab_size, "engine_set_stop: a stop id lies outside the engine's vocabulary");
    }
    TL_TRY(stop_reconcile(e));
    Pokes pk;
    const Slot &s = e->table.slots[slot];
    // the one way to resume: a decode step takes the slot again (a slot can only have stopped on an engine that armed one)
    if (s.stopped && !s.parked) pk.emplace_back(e->live + slot, 1);
    const StopRef ref{(uint64_t)(uintptr_t)(set ? set->dev : nullptr), set};
    TL_TRY(settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_stop(slot, ref, max_new_tokens, ed); }));
    if (s.stopped) e->table.resume(slot);
    return TL_OK;
}

extern "C" int tl_engine_stop_state(tl_engine *e, int slot, tl_stop_state *out) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(out, "engine_stop_state: null argument");
    TL_TRY(stop_reconcile(e));
    *out = tl_stop_state{};
    out->context = e->table.slots[slot].ctx;
    if (!e->settings.slots[slot].stop.armed) return TL_OK;
    if (!e->table.slots[slot].stopped) {  // a running slot's record: read now (a stopped slot's was read when it stopped)
        TL_TRY(aql_drain(e));
        TL_HIP(hipStreamSynchronize(e->stream));
        TL_HIP(hipMemcpy(&e->settings.slots[slot].stop_host, e->sdev<StopRecord>(SB_STOP, e->settings.at.stop_rec) + slot, sizeof(StopRecord), hipMemcpyDeviceToHost));
    }
    const StopMirror &r = e->settings.slots[slot].stop_host;
    *out = tl_stop_state{r.reason, r.index, r.generated, e->table.slots[slot].ctx, r.text_bytes, r.cut_bytes};
    return TL_OK;
}

extern "C" int tl_stop_rows(const tl_stop *set, const int32_t *tokens_dev, int rows, const int32_t *armed_dev, const int32_t *max_new_dev,
                            int32_t *automaton_dev, tl_stop_state *states_dev, void *stream) {
    TL_REQUIRE(tokens_dev && max_new_dev && automaton_dev && states_dev, "stop_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "stop_rows: rows out of range");
    static_assert(sizeof(tl_stop_state) == sizeof(StopRecord), "tl_stop_state is the device record");
    const StopArgs a{tokens_dev, 0, nullptr, set ? set->dev : nullptr, armed_dev, max_new_dev, automaton_dev, (StopRecord *)states_dev, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(stop_check_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("stop_rows");
    return TL_OK;
}

extern "C" int tl_grammar_mask_rows_stack(const tl_grammar *g, const void *logits_dev, int rows, const int32_t *states_dev, const int32_t *depths_dev,
                                          const uint64_t *stacks_dev, void *out_dev, void *stream) {
    TL_REQUIRE(g && logits_dev && states_dev && depths_dev && stacks_dev && out_dev, "grammar_mask_rows_stack: null argument");
    TL_REQUIRE(g->stack, "grammar_mask_rows_stack: not a stack grammar (tl_grammar_mask_rows)");
    TL_REQUIRE(rows > 0 && rows <= 65535, "grammar_mask_rows_stack: rows out of range");
    const GrammarStackMaskArgs a{g->dev, (const uint16_t *)logits_dev, (uint16_t *)out_dev, states_dev, depths_dev, stacks_dev, g->vocab->vocab};
    hipLaunchKernelGGL(grammar_stack_mask_rows_kernel, dim3(ceil_div(g->vocab->vocab, 2048), rows), dim3(256), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("grammar_mask_rows_stack");
    return TL_OK;
}

extern "C" int tl_grammar_mask_rows(const tl_grammar *g, const void *logits_dev, int rows, const int32_t *states_dev, void *out_dev, void *stream) {
    TL_REQUIRE(g && logits_dev && states_dev && out_dev, "grammar_mask_rows: null argument");
    TL_REQUIRE(!g->stack, "grammar_mask_rows: a stack grammar (tl_grammar_mask_rows_stack)");
    TL_REQUIRE(rows > 0 && rows <= 65535, "grammar_mask_rows: rows out of range");
    const GrammarMaskArgs a{g->dev, (const uint16_t *)logits_dev, (uint16_t *)out_dev, states_dev, g->vocab->vocab};
    hipLaunchKernelGGL(grammar_mask_rows_kernel, dim3(ceil_div(g->vocab->vocab, 2048), rows), dim3(256), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("grammar_mask_rows");
    return TL_OK;
}

extern "C" int tl_process_logits(const void *logits_dev, int rows, int vocab, const uint16_t *history_dev, const float *repetition_dev,
                                 const float *presence_dev, const float *frequency_dev, const int32_t *bias_ids_dev, const float *bias_values_dev,
                                 const int32_t *bias_n_dev, void *out_dev, void *stream) {
    TL_REQUIRE(logits_dev && history_dev && repetition_dev && presence_dev && frequency_dev && bias_n_dev && out_dev, "process_logits: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "process_logits: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "process_logits: vocabulary out of range (1 .. 524,288)");
    // (without lists every n must be 0: the kernel reads no entry then)
    const LogitProcessArgs a{(const uint16_t *)logits_dev, (uint16_t *)out_dev, vocab, 0, const_cast<uint16_t *>(history_dev), repetition_dev, presence_dev,
                             frequency_dev, bias_n_dev, bias_ids_dev, bias_values_dev, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(logit_process_kernel<false>, dim3(ceil_div(vocab, LPR_CHUNK), rows), dim3(LPR_THREADS), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("process_logits");
    return TL_OK;
}

extern "C" int tl_sample_logits(const void *logits_dev, int rows, int vocab, const float *temperature_dev, const int32_t *top_k_dev,
                                const float *top_p_dev, const uint64_t *seed_dev, const int32_t *position_dev, int32_t *ids_dev, void *stream) {
    TL_REQUIRE(logits_dev && temperature_dev && top_k_dev && top_p_dev && seed_dev && position_dev && ids_dev, "sample_logits: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "sample_logits: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "sample_logits: vocabulary out of range (1 .. 524,288)");
    hipLaunchKernelGGL(sample_rows_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, (const uint16_t *)logits_dev, vocab, temperature_dev,
                       top_k_dev, top_p_dev, seed_dev, position_dev, ids_dev);
    TL_CHECK_LAUNCH("sample_logits");
    return TL_OK;
}

extern "C" int tl_engine_set_logprobs(tl_engine *e, int slot, int top_n) {
    TL_TRY(slot_check(e, slot, false));
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_logprobs(slot, top_n, e->table.slots[slot].produced, ed); });
}

extern "C" int tl_engine_read_logprobs(tl_engine *e, int slot, int count, tl_token_logprob *out) {
    TL_TRY(slot_check(e, slot, false));
    TL_REQUIRE(out && count >= 0 && count <= e->ring_cap, "engine_read_logprobs: bad count");
    const int have = e->settings.slots[slot].lp_n < 0 ? 0 : e->table.slots[slot].produced - e->settings.slots[slot].lp_from;
    TL_REQUIRE(count <= have, "engine_read_logprobs: fewer tokens have been produced since logprobs were switched on");
    if (count == 0) return TL_OK;
    TL_HIP(hipStreamSynchronize(e->stream));
    const size_t rec = (size_t)LP_RECORD_WORDS * 4;
    const int produced = e->table.slots[slot].produced;
    std::vector<char> ring((size_t)e->ring_cap * rec);
    TL_HIP(hipMemcpy(ring.data(), e->sdev<uint32_t>(SB_LOGPROB, e->settings.at.lp_ring) + (size_t)slot * e->ring_cap * LP_RECORD_WORDS, ring.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < count; ++i) memcpy(out + i, ring.data() + (size_t)((produced - count + i) % e->ring_cap) * rec, rec);
    return TL_OK;
}

extern "C" int tl_engine_read_pending_logprobs(tl_engine *e, int count, tl_token_logprob *out) {
    TL_REQUIRE(e && out, "engine_read_pending_logprobs: null argument");
    TL_REQUIRE(count > 0 && count <= e->cfg.max_batch, "engine_read_pending_logprobs: count out of range");
    TL_REQUIRE(e->settings_mem[SB_LOGPROB], "engine_read_pending_logprobs: no slot has recorded log-probabilities (tl_engine_set_logprobs)");
    TL_HIP(hipStreamSynchronize(e->stream));
    TL_HIP(hipMemcpy(out, e->sdev<uint32_t>(SB_LOGPROB, e->settings.at.lp_pending), (size_t)count * LP_RECORD_WORDS * 4, hipMemcpyDeviceToHost));
    return TL_OK;
}

extern "C" int tl_logprob_rows(const void *logits_dev, int rows, int vocab, const int32_t *ids_dev, int top_n, float *logprob_dev,
                               int32_t *top_ids_dev, float *top_logprobs_dev, void *stream) {
    TL_REQUIRE(logits_dev && logprob_dev, "logprob_rows: null argument");
    TL_REQUIRE(rows > 0 && rows <= 65535, "logprob_rows: rows out of range");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "logprob_rows: vocabulary out of range (1 .. 524,288)");
    TL_REQUIRE(top_n >= 0 && top_n <= LP_MAX_TOP, "logprob_rows: top_n must be 0 .. 20");
    TL_REQUIRE(top_n == 0 || (top_ids_dev && top_logprobs_dev), "logprob_rows: top_n > 0 needs top_ids and top_logprobs");
    const LogprobRowsArgs a{(const uint16_t *)logits_dev, vocab, top_n, ids_dev, logprob_dev, top_ids_dev, top_logprobs_dev, nullptr};
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(rows), dim3(1024), 0, (hipStream_t)stream, a);
    TL_CHECK_LAUNCH("logprob_rows");
    return TL_OK;
}

// (the survivors between the two launches live in a block of the call's own: its release waits for the launches)
extern "C" int tl_beam_rows(const void *logits_dev, int rows, int vocab, const float *scores_dev, int n_cand, tl_beam_candidate *out_dev,
                            void *stream) {
    TL_REQUIRE(logits_dev && scores_dev && out_dev, "beam_rows: null argument");
    TL_REQUIRE(rows >= 1 && rows <= TL_MAX_BEAMS, "beam_rows: rows must be 1 .. 8");
    TL_REQUIRE(vocab > 0 && vocab <= SMP_MAX_VOCAB, "beam_rows: vocabulary out of range (1 .. 524,288)");
    TL_REQUIRE(n_cand >= 1 && n_cand <= TL_MAX_BEAM_CANDIDATES, "beam_rows: n_cand must be 1 .. 32");
    DeviceBlock survivors;
    TL_TRY(survivors.alloc(BM_SURVIVORS * sizeof(tl_beam_candidate), "beam_rows: hipMalloc(survivors) failed"));
    TL_TRY(beam_rows_launch(logits_dev, rows, vocab, scores_dev, n_cand, survivors.at<tl_beam_candidate>(), out_dev, (hipStream_t)stream));
    TL_HIP(hipStreamSynchronize((hipStream_t)stream));
    return TL_OK;
}

extern "C" int tl_pool_rows(const void *rows_dev, int hidden, int n_seqs, const int *row0, const int *len, const int *finish, const int *prior,
                            int pooling, float *sums_dev, int normalize, int dim, float *out_dev, void *stream) {
    return pool_rows((const uint16_t *)rows_dev, hidden, n_seqs, row0, len, finish, prior, nullptr, pooling, sums_dev, normalize, dim, out_dev,
                     (hipStream_t)stream);
}

// ---- the MoE kernels over caller rows (include/tinyllm_engine.h, tl_moe_route_rows / tl_moe_experts_rows) ----------------------------
extern "C" int tl_moe_route_rows(const void *logits_dev, int rows, int num_experts, int top_k, int norm_topk_prob, int32_t *ids_dev,
                                 void *scores_dev, void *stream) {
    TL_REQUIRE(logits_dev && ids_dev && scores_dev, "moe_route_rows: null argument");
    TL_REQUIRE(rows >= 1, "moe_route_rows: rows must be positive");
    TL_REQUIRE(num_experts > 0 && num_experts <= 1024 && top_k > 0 && top_k <= 16 && top_k <= num_experts,
               "moe_route_rows: need 1 <= top_k <= min(16, num_experts) and num_experts <= 1024");
    moe_route_launch((const uint16_t *)logits_dev, rows, num_experts, top_k, norm_topk_prob != 0, ids_dev, (uint16_t *)scores_dev,
                     (hipStream_t)stream);
    TL_CHECK_LAUNCH("moe_route_rows");
    return TL_OK;
}

extern "C" size_t tl_moe_experts_workspace_bytes(int rows, int top_k, int hidden, int intermediate) {
    if (rows < 1 || top_k < 1 || hidden < 1 || intermediate < 1) return 0;
    return moe_expert_rows_bytes(rows, top_k, hidden, intermediate);
}

extern "C" int tl_moe_experts_rows(const void *xn_dev, const void *h_dev, const int32_t *ids_dev, const void *scores_dev, const tl_moe_weights *w,
                                   int rows, int hidden, void *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream) {
    TL_REQUIRE(xn_dev && h_dev && ids_dev && scores_dev && w && out_dev && workspace_dev, "moe_experts_rows: null argument");
    TL_REQUIRE(w->num_experts > 0 && w->num_experts <= 1024 && w->experts_per_token > 0 && w->experts_per_token <= 16 &&
                   w->experts_per_token <= w->num_experts,
               "moe_experts_rows: need 1 <= experts_per_token <= min(16, num_experts) and num_experts <= 1024");
    TL_REQUIRE(w->intermediate_size > 0 && w->intermediate_size % 128 == 0, "moe_experts_rows: intermediate_size must be a positive multiple of 128");
    TL_REQUIRE(hidden > 0 && hidden % 128 == 0, "moe_experts_rows: hidden must be a positive multiple of 128");
    TL_REQUIRE(w->gate_dev && w->up_dev && w->down_dev && w->gate_scales_dev && w->gate_biases_dev && w->up_scales_dev && w->up_biases_dev &&
                   w->down_scales_dev && w->down_biases_dev,
               "moe_experts_rows: null expert tensor");
    TL_REQUIRE(rows >= 1 && (long)rows * w->experts_per_token <= 65535, "moe_experts_rows: rows x experts_per_token must be 1 .. 65535 (one grouped launch)");
    TL_REQUIRE(workspace_bytes >= moe_expert_rows_bytes(rows, w->experts_per_token, hidden, w->intermediate_size),
               "moe_experts_rows: the workspace is smaller than tl_moe_experts_workspace_bytes");
    TL_REQUIRE(((uintptr_t)xn_dev | (uintptr_t)h_dev | (uintptr_t)out_dev | (uintptr_t)workspace_dev) % 16 == 0, "moe_experts_rows: rows must be 16-byte aligned");
    TL_TRY(moe_experts_launch(*w, (const uint16_t *)xn_dev, (const uint16_t *)h_dev, ids_dev, (const uint16_t *)scores_dev,
                              moe_expert_rows_at(workspace_dev, rows, w->experts_per_token, w->intermediate_size), (uint16_t *)out_dev, rows, hidden,
                              (hipStream_t)stream));
    TL_CHECK_LAUNCH("moe_experts_rows");
    return TL_OK;
}

// the paged attention operator over layer l's pages, by the engine's page format
// ---- LoRA adapters (include/tinyllm_engine.h "LoRA adapters"; kernels lora.h) -----------------------------------------------------------
extern "C" int tl_engine_lora_load(tl_engine *e, const tl_lora_layer *layers, int rank, float scale, int *adapter) {
    TL_REQUIRE(e && layers && adapter, "engine_lora_load: null argument");
    TL_REQUIRE(rank >= 8 && rank <= TL_MAX_LORA_RANK && rank % 8 == 0, "engine_lora_load: rank must be a multiple of 8 up to 64");
    TL_REQUIRE(std::isfinite(scale), "engine_lora_load: scale must be finite");
    const tl_engine_config &c = e->cfg;
    const int L = c.num_layers, G = tl_engine::LORA_GROUPS;
    const int q_dim = e->q_dim(), kv_dim = c.num_kv_heads * c.head_dim, H = c.hidden_size, I = c.intermediate_size;
    // per target: its group, its segment inside the group, input and output columns
    const int t_group[TL_LORA_TARGETS] = {tl_engine::LORA_QKV, tl_engine::LORA_QKV, tl_engine::LORA_QKV, tl_engine::LORA_O,
                                          tl_engine::LORA_GU, tl_engine::LORA_GU, tl_engine::LORA_DOWN};
    const int t_seg[TL_LORA_TARGETS] = {0, 1, 2, 0, 0, 1, 0};
    const int t_in[TL_LORA_TARGETS] = {H, H, H, q_dim, H, H, I};
    const int t_out[TL_LORA_TARGETS] = {q_dim, kv_dim, kv_dim, H, I, I, H};
    bool any = false;
    for (int l = 0; l < L; ++l)
        for (int t = 0; t < TL_LORA_TARGETS; ++t) {
            const void *a = layers[l].a_dev[t], *b = layers[l].b_dev[t];
            TL_REQUIRE((a == nullptr) == (b == nullptr), "engine_lora_load: a target needs both A and B (or neither)");
            if (!a) continue;
            any = true;
            TL_REQUIRE((uintptr_t)a % 2 == 0 && (uintptr_t)b % 2 == 0, "engine_lora_load: misaligned matrix");
            if (t >= TL_LORA_GATE && e->is_moe(l)) return fail(TL_ERR_UNSUPPORTED, "engine_lora_load: MLP targets on a MoE layer are not supported");
            if (t_in[t] % 32 != 0 || t_in[t] > LORA_KS * LORA_MAX_SLICES || t_out[t] % 2 != 0)
                return fail(TL_ERR_UNSUPPORTED, "engine_lora_load: the kernels need input widths that are multiples of 32 (up to 32,768) and even output widths");
        }
    TL_REQUIRE(any, "engine_lora_load: the adapter adapts nothing");
    int id = -1;
    for (int i = 0; i < (int)e->lora_ad.size() && id < 0; ++i)
        if (!e->lora_ad[i].mem) id = i;
    if (e->lora_ad.empty()) id = 0;
    TL_REQUIRE(id >= 0, "engine_lora_load: 32 adapters are resident (tl_engine_lora_unload one first)");
    TL_TRY(aql_drain(e));
    TL_HIP(hipStreamSynchronize(e->stream));
    TL_TRY(lora_alloc(e));
    // the fused matrices: per layer and group, A = the present targets' A stacked, B [out, rank] (rows of a missing target stay zero and unread)
    std::vector<LoraDesc> descs((size_t)L * G, LoraDesc{});
    std::vector<size_t> a_off(descs.size(), 0), b_off(descs.size(), 0);
    size_t bytes = 0;
    for (int l = 0; l < L; ++l)
        for (int g = 0; g < G; ++g) {
            LoraDesc &d = descs[(size_t)l * G + g];
            d.t_off[0] = d.t_off[1] = d.t_off[2] = -1;
            int in = 0, out = 0;
            for (int t = 0; t < TL_LORA_TARGETS; ++t) {
                if (t_group[t] != g) continue;
                out += t_out[t];
                if (!layers[l].a_dev[t]) continue;
                in = t_in[t];
                d.t_off[t_seg[t]] = d.rtot;
                d.rtot += rank;
            }
            if (d.rtot == 0) continue;
            d.rank = rank, d.scale = scale;
            a_off[(size_t)l * G + g] = bytes;
            bytes = align_up(bytes + (size_t)d.rtot * in * 2, 256);
            b_off[(size_t)l * G + g] = bytes;
            bytes = align_up(bytes + (size_t)out * rank * 2, 256);
        }
    DeviceBlock block;  // the engine's once the table names it; a failure before that waits for the copies enqueued so far and releases it
    TL_TRY(block.alloc(bytes, "engine_lora_load: hipMalloc(adapter) failed"));
    char *const mem = block.at();
    const auto undo = [&](const std::string &msg) {
        (void)hipStreamSynchronize(e->stream);
        return fail(TL_ERR_HIP, "engine_lora_load: " + msg);
    };
    if (hipMemsetAsync(mem, 0, bytes, e->stream) != hipSuccess) return undo("memset failed");
    for (int l = 0; l < L; ++l)
        for (int t = 0; t < TL_LORA_TARGETS; ++t) {
            if (!layers[l].a_dev[t]) continue;
            const int g = t_group[t];
            LoraDesc &d = descs[(size_t)l * G + g];
            char *a_dst = mem + a_off[(size_t)l * G + g] + (size_t)d.t_off[t_seg[t]] * t_in[t] * 2;
            char *b_base = mem + b_off[(size_t)l * G + g];
            hipError_t rc = hipMemcpyAsync(a_dst, layers[l].a_dev[t], (size_t)rank * t_in[t] * 2, hipMemcpyDeviceToDevice, e->stream);
            const size_t row = (size_t)rank * 2;
            if (rc == hipSuccess) {
                if (g == tl_engine::LORA_GU)  // row i of gate / up -> row 2 i / 2 i + 1, like wgu
                    rc = hipMemcpy2DAsync(b_base + (size_t)t_seg[t] * row, 2 * row, layers[l].b_dev[t], row, row, (size_t)t_out[t], hipMemcpyDeviceToDevice, e->stream);
                else {
                    const size_t first = g == tl_engine::LORA_QKV ? (t == TL_LORA_Q ? 0 : (t == TL_LORA_K ? q_dim : q_dim + kv_dim)) : 0;
                    rc = hipMemcpyAsync(b_base + first * row, layers[l].b_dev[t], (size_t)t_out[t] * row, hipMemcpyDeviceToDevice, e->stream);
                }
            }
            if (rc != hipSuccess) return undo(std::string("copy failed: ") + hipGetErrorString(rc));
        }
    for (size_t i = 0; i < descs.size(); ++i)
        if (descs[i].rank > 0) descs[i].a = (const uint16_t *)(mem + a_off[i]), descs[i].b = (const uint16_t *)(mem + b_off[i]);
    if (hipStreamSynchronize(e->stream) != hipSuccess) return undo("the copies failed");
    if (hipMemcpy(e->lora_table + (size_t)id * descs.size(), descs.data(), descs.size() * sizeof(LoraDesc), hipMemcpyHostToDevice) != hipSuccess)
        return undo("hipMemcpy(table) failed");
    tl_engine::LoraResident &r = e->lora_ad[id];
    r.mem = std::move(block), r.bytes = bytes, r.rank = rank;
    r.has.assign(descs.size(), 0);
    for (size_t i = 0; i < descs.size(); ++i) r.has[i] = descs[i].rank > 0;
    *adapter = id;
    return TL_OK;
}

extern "C" int tl_engine_lora_unload(tl_engine *e, int adapter) {
    TL_REQUIRE(e, "engine_lora_unload: null engine");
    TL_REQUIRE(adapter >= 0 && adapter < (int)e->lora_ad.size() && e->lora_ad[adapter].mem, "engine_lora_unload: no such adapter");
    for (int s = 0; s < e->cfg.max_batch; ++s)
        TL_REQUIRE(e->settings.slots[s].lora != adapter, "engine_lora_unload: a live or parked slot carries the adapter (release it first)");
    TL_TRY(aql_drain(e));
    TL_HIP(hipStreamSynchronize(e->stream));
    const size_t n = (size_t)e->cfg.num_layers * tl_engine::LORA_GROUPS;
    TL_HIP(hipMemset(e->lora_table + (size_t)adapter * n, 0, n * sizeof(LoraDesc)));
    TL_HIP(hipDeviceSynchronize());
    e->lora_ad[adapter] = tl_engine::LoraResident{};
    return TL_OK;
}

extern "C" int tl_engine_set_lora(tl_engine *e, int slot, int adapter) {
    TL_TRY(slot_check(e, slot, true));
    TL_REQUIRE(adapter == LORA_NONE || (adapter >= 0 && adapter < (int)e->lora_ad.size() && e->lora_ad[adapter].mem),
               "engine_set_lora: the adapter is -1 (none) or the id of a resident adapter");
    TL_REQUIRE(e->table.slots[slot].ctx == 0 && e->table.slots[slot].pages.empty(),
               "engine_set_lora: the slot already holds tokens (a sequence's K/V are all computed under one adapter: set it before the first prefill)");
    Pokes pk;
    return settings_set(e, slot, pk, [&](SettingsEdits &ed) { return e->settings.set_lora(slot, adapter, ed); });
}

extern "C" int tl_engine_slot_lora(const tl_engine *e, int slot) {
    if (!e || slot < 0 || slot >= e->cfg.max_batch) return LORA_NONE;
    return e->settings.slots[slot].lora;
}

extern "C" int tl_engine_lora_stats(const tl_engine *e, tl_lora_stats *out) {
    TL_REQUIRE(e && out, "engine_lora_stats: null argument");
    *out = tl_lora_stats{};
    for (const tl_engine::LoraResident &r : e->lora_ad)
        if (r.mem) out->resident += 1, out->bytes += r.bytes;
    out->adapter_steps = e->lora_steps;
    out->adapter_prefill_rows = e->lora_prefill_rows;
    return TL_OK;
}

extern "C" int tl_lora_rows(const void *x_dev, int rows, int in, int out, const int32_t *row_adapter_dev, const tl_lora_matrices *adapters, int n_adapters,
                            int seg_mode, int seg_end0, int seg_end1, const int *tile_row0, const int *tile_rows, const int *tile_adapter, int n_tiles,
                            int mode, const void *base_or_residual_dev, void *out_dev, const void *norm_w_dev, float eps, void *stream) {
    TL_REQUIRE(x_dev && out_dev && adapters, "lora_rows: null argument");
    TL_REQUIRE(rows >= 1 && n_adapters >= 1 && n_adapters <= TL_MAX_LORA_ADAPTERS, "lora_rows: at least one row and 1 .. 32 adapters");
    TL_REQUIRE(seg_mode >= LORA_SEG_PLAIN && seg_mode <= LORA_SEG_INTERLEAVED, "lora_rows: seg_mode is 0 (one segment), 1 (three blocks) or 2 (interleaved)");
    TL_REQUIRE(seg_mode != LORA_SEG_BLOCKS || (0 <= seg_end0 && seg_end0 <= seg_end1 && seg_end1 <= out), "lora_rows: block ends out of order");
    const int n_seg = seg_mode == LORA_SEG_BLOCKS ? 3 : (seg_mode == LORA_SEG_INTERLEAVED ? 2 : 1);
    std::vector<LoraDesc> descs(n_adapters, LoraDesc{});
    for (int i = 0; i < n_adapters; ++i) {
        const tl_lora_matrices &m = adapters[i];
        LoraDesc &d = descs[i];
        TL_REQUIRE(m.a_dev && m.b_dev && (uintptr_t)m.a_dev % 16 == 0 && (uintptr_t)m.b_dev % 16 == 0, "lora_rows: adapter matrices must be 16-byte aligned");
        TL_REQUIRE(m.rank >= 8 && m.rank <= TL_MAX_LORA_RANK && m.rank % 8 == 0, "lora_rows: rank must be a multiple of 8 up to 64");
        TL_REQUIRE(std::isfinite(m.scale), "lora_rows: scale must be finite");
        TL_REQUIRE(m.seg_mask > 0 && m.seg_mask < (1 << n_seg), "lora_rows: seg_mask names no segment, or one the layout does not have");
        d.a = (const uint16_t *)m.a_dev, d.b = (const uint16_t *)m.b_dev, d.scale = m.scale, d.rank = m.rank;
        for (int s = 0; s < 3; ++s) {
            d.t_off[s] = -1;
            if (s < n_seg && ((m.seg_mask >> s) & 1)) d.t_off[s] = d.rtot, d.rtot += m.rank;
        }
    }
    std::vector<LoraTile> tiles;
    bool looks_up = n_tiles == 0;
    if (n_tiles == 0) lora_lookup_tiles(rows, tiles);
    else {
        TL_REQUIRE(n_tiles > 0 && tile_row0 && tile_rows && tile_adapter, "lora_rows: a tile list needs its three arrays");
        for (int i = 0; i < n_tiles; ++i) {
            TL_REQUIRE(tile_row0[i] >= 0 && tile_rows[i] >= 0 && tile_rows[i] <= LORA_TILE && (long)tile_row0[i] + tile_rows[i] <= rows,
                       "lora_rows: a tile is up to 16 rows inside [0, rows)");
            TL_REQUIRE(tile_adapter[i] >= LORA_ROW_LOOKUP && tile_adapter[i] < n_adapters, "lora_rows: a tile's adapter is -2 (per row), -1 (none) or an index");
            looks_up = looks_up || tile_adapter[i] == LORA_ROW_LOOKUP;
            tiles.push_back(LoraTile{tile_row0[i], tile_rows[i], tile_adapter[i], 0});
        }
    }
    TL_REQUIRE(!looks_up || row_adapter_dev, "lora_rows: tiles that look their rows' adapters up need row_adapter_dev");
    const int nt = (int)tiles.size();
    Carve carve;
    const size_t o_table = carve(descs.size() * sizeof(LoraDesc)), o_tiles = carve(tiles.size() * sizeof(LoraTile));
    const size_t o_part = carve(lora_partial_floats(nt, std::max(in, 1)) * 4), o_ss = carve(lora_ss_floats(nt, std::max(in, 1)) * 4);
    DeviceBlock ws;  // (released behind the synchronisation below)
    TL_TRY(ws.alloc(carve.off, "lora_rows: hipMalloc(workspace) failed"));
    char *const mem = ws.at();
    int rc = TL_OK;
    if (hipMemcpy(mem + o_table, descs.data(), descs.size() * sizeof(LoraDesc), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(mem + o_tiles, tiles.data(), tiles.size() * sizeof(LoraTile), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(TL_ERR_HIP, "lora_rows: hipMemcpy(table) failed");
    if (rc == TL_OK) {
        LoraCall c;
        c.table = (const LoraDesc *)(mem + o_table), c.stride = 1, c.index = 0, c.n_adapters = n_adapters, c.row_adapter = row_adapter_dev;
        c.tiles_dev = (const LoraTile *)(mem + o_tiles), c.n_tiles = nt, c.total_rows = rows, c.x = (const uint16_t *)x_dev, c.in = in, c.out = out;
        c.norm_w = (const uint16_t *)norm_w_dev, c.eps = eps, c.partial = (float *)(mem + o_part), c.ss = (float *)(mem + o_ss);
        c.seg_mode = seg_mode, c.seg_end0 = seg_end0, c.seg_end1 = seg_end1, c.mode = mode;
        c.base = (const uint16_t *)base_or_residual_dev, c.dst = (uint16_t *)out_dev;
        rc = lora_apply(c, (hipStream_t)stream);
    }
    const hipError_t se = hipStreamSynchronize((hipStream_t)stream);
    if (rc == TL_OK && se != hipSuccess) rc = fail(TL_ERR_HIP, std::string("lora_rows: ") + hipGetErrorString(se));
    return rc;
}

static int engine_paged_attention(tl_engine *e, int l, const uint16_t *q_t, const int32_t *block_row, const int32_t *ctx_dev, uint16_t *attn_t,
                                  int n, int ctx_hint) {
    const tl_engine_config &c = e->cfg;
    const int D = c.head_dim, Hq = c.num_heads, Hkv = c.num_kv_heads;
    if (e->kv_format == TL_KV_FP8_E4M3)
        return tl_paged_attention_fp8(q_t, e->layer_k(l), e->layer_ks(l), e->layer_v(l), e->layer_vs(l), block_row, ctx_dev, attn_t, Hq, n, D,
                                      c.num_pages, c.page_size, c.max_pages_per_seq, Hq, Hkv, 1.0f / sqrtf((float)D), 1, ctx_hint, e->shared.attn_ws,
                                      e->attn.ws_bytes, e->stream);
    return tl_paged_attention(q_t, e->layer_k(l), e->layer_v(l), block_row, ctx_dev, attn_t, Hq, n, D, c.num_pages, c.page_size,
                              c.max_pages_per_seq, Hq, Hkv, 1.0f / sqrtf((float)D), 1, ctx_hint, TL_BF16, e->shared.attn_ws, e->attn.ws_bytes, e->stream);
}
static void launch_qkv_post(tl_engine *e, int l, QkvPostArgs &q, int n) {
    q.key_scales = e->layer_ks(l);
    q.value_scales = e->layer_vs(l);
    switch (e->cfg.head_dim) {
        case 128:
            if (e->kv_format == TL_KV_FP8_E4M3) hipLaunchKernelGGL((qkv_post_kernel<8, true>), dim3(n), dim3(256), 0, e->stream, q);
            else hipLaunchKernelGGL((qkv_post_kernel<8>), dim3(n), dim3(256), 0, e->stream, q);
            break;
        case 64: hipLaunchKernelGGL((qkv_post_kernel<4>), dim3(n), dim3(256), 0, e->stream, q); break;
        default: hipLaunchKernelGGL((qkv_post_kernel<2>), dim3(n), dim3(256), 0, e->stream, q); break;
    }
}

// One sequence's chunk in a prefill pass: its slot, the position of its first token, its first row among the pass's rows, its length
struct PrefillSeq {
    int slot, start, row0, len;
};

// the lm_head over `rows` rows of the residual stream through the GEMV with the final RMSNorm fused (a prefill's last rows, verification)
static int lm_head_rows(tl_engine *e, const uint16_t *x, int rows) {
    Proj p = proj(e->head(), x, e->logits, rows);
    p.pro = PRO_RMSNORM, p.norm_w = e->final_norm;
    return engine_qmv(e->lin, p);
}

// The multi-token pass over the `total` rows of the chunks in `seqs`, side by side: their pages reserved (the caller has checked
// whatever could fail part way) and their tokens embedded, then every layer -- the projections once over all rows, RoPE / KV append, the
// paged FlashAttention and the head transpose per sequence (each has its own block-table row, start position and causal mask) -- and
// the slots' context lengths advanced.  The last layer's rows stay in x.  `packed` names the caller in the errors.
static int prefill_pass(tl_engine *e, const PrefillSeq *seqs, int n_seqs, const int32_t *tokens, int total, bool packed) {
    const tl_engine_config &c = e->cfg;
    const Act &b = e->shared;  // every layer hands over in the shared buffers
    SlotEdits ed;
    Pokes pk;
    for (int i = 0; i < n_seqs; ++i) {
        TL_TRY(table_rc(e->table.reserve(seqs[i].slot, seqs[i].start + seqs[i].len, ed)));
        pk.emplace_back(e->scratch_ctx + i, seqs[i].start + seqs[i].len);
    }
    TL_TRY(apply_edits(e, ed, pk));
    TL_TRY(poke(e, pk));
    TL_HIP(hipMemcpyAsync(e->prefill_tokens, tokens, (size_t)total * 4, hipMemcpyHostToDevice, e->stream));
    for (int i = 0; i < n_seqs; ++i) {  // ... and the sequence row of a slot that records its ids (dry.h)
        if (!step_records_slot(e, seqs[i].slot)) continue;
        launch_dry_record(e, seqs[i].slot, e->prefill_tokens + seqs[i].row0, seqs[i].len, seqs[i].start);
        TL_CHECK_LAUNCH("engine sequence recording");
    }
    for (int i = 0; i < n_seqs; ++i)  // ... and the history row of a slot armed for prompt lookup (lookup.h)
        TL_TRY(lookup_record_chunk(e, seqs[i].slot, e->prefill_tokens + seqs[i].row0, seqs[i].len, seqs[i].start));
    for (int i = 0; i < n_seqs; ++i) {  // the chunk's tokens enter the history of a slot that processes its logits (logit_process.h)
        if (!step_processes_slot(e, seqs[i].slot)) continue;
        const LogitMarkArgs mk{e->prefill_tokens + seqs[i].row0, seqs[i].len, c.vocab_size, e->sdev<uint32_t>(SB_PROCESS, e->settings.at.pen_history), (long)seqs[i].slot * c.vocab_size};
        hipLaunchKernelGGL(logit_mark_prompt_kernel, dim3(ceil_div(seqs[i].len, 256)), dim3(256), 0, e->stream, mk);
        TL_CHECK_LAUNCH("engine prompt marking");
    }

    const int D = c.head_dim, Hq = c.num_heads, Hkv = c.num_kv_heads;
    TL_TRY(tl_quantized_embedding(e->prefill_tokens, 0, e->embed.scales_dev, e->embed.biases_dev, e->embed.weight_dev, b.x_out,
                                  total, c.hidden_size, c.vocab_size, 128, 4, TL_BF16, e->stream));
    for (int i = 0; i < n_seqs; ++i)
        TL_REQUIRE(tl_paged_attention_workspace_bytes(Hq, seqs[i].len, D, c.page_size, c.max_pages_per_seq, Hq, Hkv, seqs[i].start + seqs[i].len) <=
                       e->attn.ws_bytes, std::string(packed ? "engine_prefill_packed" : "engine_prefill") + ": attention workspace too small");
    // a pass in which some sequence carries a LoRA adapter (lora.h): tiles of 16 rows that never straddle two sequences, written here;
    // lora_on(l, g): some sequence's adapter adapts group g of layer l -- the shrink / expand launches run around that projection
    int lora_tiles = 0;
    std::vector<LoraTile> lora_list;
    {
        int row0[PACKED_MAX_SEQS], len[PACKED_MAX_SEQS], ad[PACKED_MAX_SEQS];
        bool any = false;
        for (int i = 0; i < n_seqs; ++i) {
            row0[i] = seqs[i].row0, len[i] = seqs[i].len, ad[i] = e->settings.slots[seqs[i].slot].lora;
            if (ad[i] >= 0) any = true, e->lora_prefill_rows += seqs[i].len;
        }
        if (any) {
            TL_REQUIRE(lora_build_tiles(n_seqs, row0, len, ad, lora_list) && (int)lora_list.size() <= lora_tiles_cap(e), "engine: bad LoRA tile list");
            lora_tiles = (int)lora_list.size();
            TL_HIP(hipMemcpyAsync(e->lora_tiles_prefill, lora_list.data(), lora_list.size() * sizeof(LoraTile), hipMemcpyHostToDevice, e->stream));
        }
    }
    const auto lora_on = [&](int l, int g) {
        if (lora_tiles == 0) return false;
        for (int i = 0; i < n_seqs; ++i) {
            const int a = e->settings.slots[seqs[i].slot].lora;
            if (a >= 0 && e->lora_ad[a].has[(size_t)l * tl_engine::LORA_GROUPS + g]) return true;
        }
        return false;
    };
    bool x_normed = false;  // the previous layer's w_down reduction left this layer's normalised rows in xn (engine_gemm)
    for (int l = 0; l < c.num_layers; ++l) {
        const tl_layer_weights &w = e->layers[l];
        if (!x_normed) TL_TRY(tl_rms_norm(b.x_out, w.input_norm_dev, b.xn, total, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
        x_normed = false;
        TL_TRY(engine_gemm(e->lin, proj(w.wqkv, b.xn, b.qkv, total)));
        if (lora_on(l, tl_engine::LORA_QKV))
            TL_TRY(lora_group(e, l, tl_engine::LORA_QKV, e->lora_tiles_prefill, lora_tiles, total, b.xn, nullptr, TL_LORA_ADD, nullptr, b.qkv));
        for (int i = 0; i < n_seqs; ++i) {
            const int n = seqs[i].len, start = seqs[i].start;
            const int32_t *block_row = e->block_table + (size_t)seqs[i].slot * c.max_pages_per_seq;
            uint16_t *q_t = e->q_t + (size_t)seqs[i].row0 * Hq * D;  // this sequence's [Hq][n][D] block
            uint16_t *attn_t = e->attn_t + (size_t)seqs[i].row0 * Hq * D;
            QkvPostArgs q{};
            q.qkv = b.qkv + (size_t)seqs[i].row0 * (Hq + 2 * Hkv) * D;
            q.q_norm_w = (const uint16_t *)w.q_norm_dev;
            q.k_norm_w = (const uint16_t *)w.k_norm_dev;
            q.q_t = q_t;
            q.key_pages = e->layer_k(l);
            q.value_pages = e->layer_v(l);
            q.block_row = block_row;
            q.T = n;
            q.start = start;
            q.page_size = c.page_size;
            q.max_pages = c.max_pages_per_seq;
            q.num_heads = Hq;
            q.num_kv_heads = Hkv;
            q.eps = c.rms_norm_eps;
            q.rope_base = c.rope_theta;
            launch_qkv_post(e, l, q, n);
            TL_CHECK_LAUNCH("engine qkv_post");
            TL_TRY(engine_paged_attention(e, l, q_t, block_row, e->scratch_ctx + i, attn_t, n, start + n));
            const long items = (long)Hq * n * (D / 8);
            hipLaunchKernelGGL(heads_to_rows_kernel, dim3(ceil_div(items, 256)), dim3(256), 0, e->stream, attn_t,
                               b.attn + (size_t)seqs[i].row0 * Hq * D, Hq, n, D);
        }
        bool h_normed = false;
        Proj po = proj(w.wo, b.attn, b.h, total);
        po.epi = EPI_RESIDUAL, po.residual = b.x_out, po.norm_out = w.post_norm_dev, po.out_w = b.xn;
        if (lora_on(l, tl_engine::LORA_O)) {  // x + delta first: the projection's residual epilogue then adds its product to that
            TL_TRY(lora_group(e, l, tl_engine::LORA_O, e->lora_tiles_prefill, lora_tiles, total, b.attn, nullptr, TL_LORA_RESIDUAL_PRE, b.x_out, e->lora_tmp));
            po.residual = e->lora_tmp;
        }
        TL_TRY(engine_gemm(e->lin, po, &h_normed));
        if (!h_normed) TL_TRY(tl_rms_norm(b.h, w.post_norm_dev, b.xn, total, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
        if (e->is_moe(l)) {
            TL_TRY(engine_moe_mlp(e, l, b.xn, b.h, b.x_out, total, nullptr));
        } else {
            TL_REQUIRE(w.wgu.weight_dev != nullptr, "engine: a layer has neither a dense MLP nor experts (tl_engine_set_moe_layer)");
            Proj pg = proj(w.wgu, b.xn, b.act, total);
            pg.epi = EPI_SWIGLU;
            if (lora_on(l, tl_engine::LORA_GU)) {  // the unfused route: complete gate|up rows, then the expand launch's SwiGLU over base + delta
                pg.out = e->lin.gu, pg.epi = EPI_STORE;
                TL_TRY(engine_gemm(e->lin, pg));
                TL_TRY(lora_group(e, l, tl_engine::LORA_GU, e->lora_tiles_prefill, lora_tiles, total, b.xn, nullptr, TL_LORA_SWIGLU, e->lin.gu, b.act));
            } else {
                TL_TRY(engine_gemm(e->lin, pg));
            }
            Proj pd = proj(w.wdown, b.act, b.x_out, total);
            pd.epi = EPI_RESIDUAL, pd.residual = b.h, pd.norm_out = l + 1 < c.num_layers ? e->layers[l + 1].input_norm_dev : nullptr, pd.out_w = b.xn;
            if (lora_on(l, tl_engine::LORA_DOWN)) {
                TL_TRY(lora_group(e, l, tl_engine::LORA_DOWN, e->lora_tiles_prefill, lora_tiles, total, b.act, nullptr, TL_LORA_RESIDUAL_PRE, b.h, e->lora_tmp));
                pd.residual = e->lora_tmp;
            }
            TL_TRY(engine_gemm(e->lin, pd, &x_normed));
        }
        TL_CHECK_LAUNCH(packed ? "engine packed prefill layer" : "engine prefill layer");
    }
    for (int i = 0; i < n_seqs; ++i) {
        // (seqs[i].start is the slot's context; the ids of a slot with a LoRA adapter stay unknown to the prefix cache: its K/V are the adapter's)
        e->table.appended(seqs[i].slot, tokens + seqs[i].row0, seqs[i].len, !e->lora_slot(seqs[i].slot));
        e->settings.appended(seqs[i].slot, true);  // a pending token that is prefilled past is never fed (an embedding keeps its mean: embed_pool)
        pk.emplace_back(e->context_lens + seqs[i].slot, seqs[i].start + seqs[i].len);
    }
    TL_TRY(poke(e, pk));
    e->stats.prefill_tokens += total;
    return TL_OK;
}

// The first token of a prefilled slot from row `row` of the logits: the chain behind the lm_head (advance 0: the prefill has set the
// context length), after which the slot has produced one id.  Its embedding row goes to scratch: the prefill activations in x must stay
// intact; decode re-embeds from tokens
static int prefill_first_token(tl_engine *e, int slot, int row, const char *what) {
    launch_logit_chain(e, e->logits + (size_t)row * e->cfg.vocab_size, row, 1, slot, 0, e->shared.h, nullptr, 0, nullptr, nullptr, step_features(e, slot, 1), nullptr);
    TL_CHECK_LAUNCH(what);
    e->table.slots[slot].produced += 1;
    e->settings.pending_produced(slot);
    return TL_OK;
}

// logits_mode: 0 = none, 1 = last row (greedy id recorded as the slot's pending token), 2 = every row (n <= 8: greedy ids
// land in e->verify_ids, nothing is recorded; speculative verification), 3 = every row scored (tl_engine_score: the log-probability
// of e->score_ids[i] and the greedy id of every row into e->score_lp / e->score_argmax, nothing recorded, e->logits untouched)
static int prefill_impl(tl_engine *e, int slot, const int32_t *tokens, int n, int logits_mode) {
    TL_TRY(slot_check_feeds(e, slot));
    TL_REQUIRE(tokens && n > 0, "engine_prefill: need at least one token");
    TL_REQUIRE(n <= e->cfg.max_prefill_rows, "engine_prefill: chunk exceeds max_prefill_rows");
    const tl_engine_config &c = e->cfg;
    TL_REQUIRE(n <= 8 || c.head_dim == 128, "engine_prefill: chunks longer than 8 tokens need head_dim 128 (bf16 FlashAttention)");
    for (int i = 0; i < n; ++i) TL_REQUIRE(tokens[i] >= 0 && tokens[i] < c.vocab_size, "engine_prefill: token id out of range");
    const PrefillSeq seq{slot, e->table.slots[slot].ctx, 0, n};
    TL_TRY(prefill_pass(e, &seq, 1, tokens, n, false));
    if (logits_mode == 3) {
        // the final RMSNorm over the chunk's rows, then the lm_head through the W4 GEMM a block of rows at a time into the scoring
        // scratch, each block followed by the logprob routine in gather mode
        TL_TRY(tl_rms_norm(e->shared.x_out, e->final_norm, e->shared.xn, n, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
        for (int r0 = 0; r0 < n; r0 += SCORE_BLOCK_ROWS) {
            const int rows = std::min(SCORE_BLOCK_ROWS, n - r0);
            TL_TRY(engine_gemm(e->lin, proj(e->head(), e->shared.xn + (size_t)r0 * c.hidden_size, e->score_logits, rows)));
            const LogprobRowsArgs a{e->score_logits, c.vocab_size, 0, e->score_ids + r0, e->score_lp + r0, nullptr, nullptr, e->score_argmax + r0};
            hipLaunchKernelGGL(logprob_rows_kernel, dim3(rows), dim3(1024), 0, e->stream, a);
            TL_CHECK_LAUNCH("engine score logprobs");
        }
    }
    if (logits_mode == 2) {
        TL_TRY(lm_head_rows(e, e->shared.x_out, n));
        e->logits_rows = n, e->logits_slot = slot;
        hipLaunchKernelGGL(argmax_rows_kernel, dim3(n), dim3(1024), 0, e->stream, e->logits, c.vocab_size, e->verify_ids);
        TL_CHECK_LAUNCH("engine verify argmax");
    }
    if (logits_mode == 1) {
        // logits_to_keep = 1 (reference qwen3_week3.py:331-336): last row only
        const uint16_t *last = e->shared.x_out + (size_t)(n - 1) * c.hidden_size;
        TL_TRY(lm_head_rows(e, last, 1));
        e->logits_rows = 1, e->logits_slot = slot;
        TL_TRY(prefill_first_token(e, slot, 0, "engine prefill argmax"));
    }
    return TL_OK;
}

// What the passes over several sequences' chunks check alike, all before anything is reserved or allocated, and the pass's sequences with
// the sum of their rows.  Per sequence: the slot feeds, the caller's own refusal (`per_seq(i)`), no slot twice, the pages its chunk needs
// -- with `commit` one more where a rewind into a page the chunk filled copies it (SlotTable::rewind, when the prefix index has taken
// it).  Then the caller's limits on the sum (`limits(total)`), the page pool and the token range.  `w` starts every message.
template <class PerSeq, class Limits>
static int pass_seqs(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, bool commit, const std::string &w, PerSeq per_seq,
                     Limits limits, std::vector<PrefillSeq> &seqs, int *total) {
    const tl_engine_config &c = e->cfg;
    std::vector<PrefillSeq> list(n_seqs);
    int rows = 0;
    size_t extra_pages = 0;
    for (int i = 0; i < n_seqs; ++i) {
        TL_TRY(slot_check_feeds(e, slots[i]));
        TL_TRY(per_seq(i));
        for (int j = 0; j < i; ++j) TL_REQUIRE(slots[j] != slots[i], w + "a slot appears twice");
        const Slot &s = e->table.slots[slots[i]];
        const int need = (s.ctx + lens[i] + c.page_size - 1) / c.page_size;
        TL_REQUIRE(need <= c.max_pages_per_seq, "engine: sequence exceeds max_pages_per_seq * page_size tokens");
        if (need > (int)s.pages.size()) extra_pages += (size_t)need - s.pages.size();
        if (commit && lens[i] > 1 && e->table.pool.enabled && (s.ctx + lens[i]) / c.page_size > s.ctx / c.page_size) extra_pages += 1;
        list[i] = {slots[i], s.ctx, rows, lens[i]};
        rows += lens[i];
    }
    TL_TRY(limits(rows));
    TL_REQUIRE(e->table.pool.can_take(extra_pages), "engine: KV page pool exhausted");  // checked before anything is mutated
    for (int i = 0; i < rows; ++i) TL_REQUIRE(tokens[i] >= 0 && tokens[i] < c.vocab_size, w + "token id out of range");
    seqs = std::move(list);
    *total = rows;
    return TL_OK;
}

// The checks of a packed pass and the pass's sequences: `ends` (may be NULL: none) marks the chunks that want a logits row.  `what` names
// the caller in the errors.
static int packed_seqs(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, const int *ends, const char *what,
                       std::vector<PrefillSeq> &seqs, int *total) {
    const tl_engine_config &c = e->cfg;
    const std::string w = std::string(what) + ": ";
    TL_REQUIRE(n_seqs >= 1 && n_seqs <= PACKED_MAX_SEQS, w + "between 1 and 16 sequences per call");
    TL_REQUIRE(c.head_dim == 128, w + "head_dim 128 (bf16 FlashAttention)");
    const auto per_seq = [&](int i) {
        TL_REQUIRE(lens[i] > 0, w + "every sequence needs at least one token");
        return (int)TL_OK;
    };
    const auto limits = [&](int rows) {
        TL_REQUIRE(rows <= c.max_prefill_rows, w + "the chunks together exceed max_prefill_rows");
        int wanted = 0;
        for (int i = 0; ends && i < n_seqs; ++i) wanted += ends[i] ? 1 : 0;
        TL_REQUIRE(wanted <= logits_rows(c.max_batch), w + "more prompts end in this pass than the logits buffer has rows (max(max_batch, 8))");
        return (int)TL_OK;
    };
    return pass_seqs(e, n_seqs, slots, tokens, lens, false, w, per_seq, limits, seqs, total);
}

// Several sequences' chunks in ONE prefill pass: the projections (97 % of the prefill FLOPs) run once over the concatenated rows -- a
// 2,048-row GEMM instead of several 300-row ones.
static int prefill_packed_impl(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, const int *want_logits) {
    const tl_engine_config &c = e->cfg;
    TL_REQUIRE(e && slots && tokens && lens && want_logits, "engine_prefill_packed: null argument");
    std::vector<PrefillSeq> seqs;
    int total = 0;
    TL_TRY(packed_seqs(e, n_seqs, slots, tokens, lens, want_logits, "engine_prefill_packed", seqs, &total));
    TL_TRY(prefill_pass(e, seqs.data(), n_seqs, tokens, total, true));
    int n_logits = 0;
    for (int i = 0; i < n_seqs; ++i) {
        if (!want_logits[i]) continue;
        // last rows side by side in xn: one lm_head pass over them (logits_to_keep = 1, qwen3_week3.py:331-336)
        TL_HIP(hipMemcpyAsync(e->shared.xn + (size_t)n_logits * c.hidden_size, e->shared.x_out + (size_t)(seqs[i].row0 + lens[i] - 1) * c.hidden_size,
                              (size_t)c.hidden_size * 2, hipMemcpyDeviceToDevice, e->stream));
        ++n_logits;
    }
    if (n_logits > 0) {
        TL_TRY(lm_head_rows(e, e->shared.xn, n_logits));
        e->logits_rows = n_logits, e->logits_slot = -2;
        int j = 0;
        for (int i = 0; i < n_seqs; ++i) {
            if (!want_logits[i]) continue;
            TL_TRY(prefill_first_token(e, slots[i], j, "engine packed prefill argmax"));
            ++j;
        }
    }
    return TL_OK;
}

extern "C" int tl_engine_prefill_packed(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens,
                                        const int *want_logits) {
    TL_REQUIRE(e, "engine_prefill_packed: null engine");
    return prefill_packed_impl(e, n_seqs, slots, tokens, lens, want_logits);
}

extern "C" int tl_engine_prefill(tl_engine *e, int slot, const int32_t *tokens, int n, int want_logits) {
    return prefill_impl(e, slot, tokens, n, want_logits ? 1 : 0);
}

extern "C" int tl_engine_score(tl_engine *e, int slot, const int32_t *tokens, int n, int32_t next_token, float *out_logprobs,
                               int32_t *out_argmax) {
    TL_REQUIRE(e && tokens && out_logprobs, "engine_score: null argument");
    TL_REQUIRE(n >= 1 && n <= e->cfg.max_prefill_rows, "engine_score: between 1 and max_prefill_rows tokens per call");
    TL_REQUIRE(next_token < e->cfg.vocab_size, "engine_score: next_token out of range");
    TL_REQUIRE(e->cfg.vocab_size <= SMP_MAX_VOCAB, "engine_score: vocabulary larger than the routine's 524,288 tokens");
    TL_TRY(slot_check_feeds(e, slot));
    if (!e->score_logits) {
        const size_t R = (size_t)e->cfg.max_prefill_rows, logit_bytes = align_up((size_t)SCORE_BLOCK_ROWS * e->cfg.vocab_size * 2, 256);
        TL_TRY(e->score_mem.alloc(logit_bytes + R * 12, "engine_score: hipMalloc(scratch) failed"));
        e->score_logits = e->score_mem.at<uint16_t>();
        e->score_ids = e->score_mem.at<int32_t>(logit_bytes);
        e->score_lp = (float *)(e->score_ids + R);
        e->score_argmax = e->score_ids + 2 * R;
    }
    std::vector<int32_t> targets(tokens + 1, tokens + n);
    targets.push_back(next_token < 0 ? -1 : next_token);
    TL_HIP(hipMemcpyAsync(e->score_ids, targets.data(), (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
    TL_TRY(prefill_impl(e, slot, tokens, n, 3));
    TL_HIP(hipMemcpyAsync(out_logprobs, e->score_lp, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    if (out_argmax) TL_HIP(hipMemcpyAsync(out_argmax, e->score_argmax, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    return TL_OK;
}

// ---- embeddings (include/tinyllm_engine.h "Embeddings"; the kernels are pool.h) -----------------------------------------------------------
// what an embed call checks before it looks at a slot
static int embed_args_check(const tl_engine *e, int pooling, int dim, bool finishes, const float *out_host) {
    TL_REQUIRE(pooling == TL_POOL_LAST || pooling == TL_POOL_MEAN, "engine_embed: pooling is TL_POOL_LAST or TL_POOL_MEAN");
    TL_REQUIRE(dim >= 1 && dim <= e->cfg.hidden_size, "engine_embed: dim must be 1 .. hidden_size");
    TL_REQUIRE(e->cfg.hidden_size % 2 == 0, "engine_embed: hidden_size must be even");
    TL_REQUIRE(!finishes || out_host, "engine_embed: a text finishes and out_host is null");
    return TL_OK;
}
// MEAN: every chunk restarts its slot's running sum at context 0 or continues it at exactly the rows the sum holds
static int embed_mean_check(const tl_engine *e, const PrefillSeq *seqs, int n_seqs) {
    for (int i = 0; i < n_seqs; ++i)
        TL_REQUIRE(seqs[i].start == 0 || e->settings.slots[seqs[i].slot].emb_rows == seqs[i].start,
                   "engine_embed: mean pooling continues a text embedded from context 0 with TL_POOL_MEAN chunks only (the slot's context came from elsewhere)");
    return TL_OK;
}
static int embed_alloc(tl_engine *e, bool mean) {
    const size_t H = (size_t)e->cfg.hidden_size;
    if (!e->emb_out) {
        const size_t bytes = POOL_MAX_SEQS * H * sizeof(float);
        TL_TRY(e->emb_out_mem.alloc(bytes, "engine_embed: hipMalloc(vectors) failed"));
        e->emb_out = e->emb_out_mem.at<float>();
        e->stats.workspace_bytes += bytes;
    }
    if (mean && !e->emb_sums) {
        const size_t bytes = (size_t)e->cfg.max_batch * H * sizeof(float);
        TL_TRY(e->emb_sums_mem.alloc(bytes, "engine_embed: hipMalloc(running sums) failed"));
        e->emb_sums = e->emb_sums_mem.at<float>();
        e->stats.workspace_bytes += bytes;
    }
    return TL_OK;
}
// The pooling stage behind a prefill pass whose rows are still in x.  LAST: the finishing sequences' last rows side by side in h (as
// prefill_packed_impl gathers the rows of the lm_head), the final RMSNorm over those, the finish.  MEAN: the final RMSNorm over every
// row of the pass (as tl_engine_score), the column sums into the slots' running sums, the finish.  Synchronises when a text finishes.
static int embed_pool(tl_engine *e, const PrefillSeq *seqs, int n_seqs, const int *finish, int pooling, int normalize, int dim, float *out_host) {
    const tl_engine_config &c = e->cfg;
    const size_t H = (size_t)c.hidden_size;
    const bool mean = pooling == TL_POOL_MEAN;
    TL_TRY(embed_alloc(e, mean));
    int row0[POOL_MAX_SEQS], len[POOL_MAX_SEQS], prior[POOL_MAX_SEQS], sum_index[POOL_MAX_SEQS], fin[POOL_MAX_SEQS];
    int n = 0, n_finish = 0, total = 0;
    for (int i = 0; i < n_seqs; ++i) {
        const PrefillSeq &q = seqs[i];
        total += q.len;
        if (mean) {
            row0[n] = q.row0, len[n] = q.len, sum_index[n] = q.slot, fin[n] = finish[i] ? 1 : 0;
            prior[n] = q.start == 0 ? 0 : e->settings.slots[q.slot].emb_rows;
            e->settings.slots[q.slot].emb_rows = prior[n] + q.len;
            n_finish += fin[n++];
            continue;
        }
        e->settings.rewound(q.slot);  // (a LAST chunk: the context no longer is a running mean's)
        if (!finish[i]) continue;
        TL_HIP(hipMemcpyAsync(e->shared.h + (size_t)n * H, e->shared.x_out + (size_t)(q.row0 + q.len - 1) * H, H * 2, hipMemcpyDeviceToDevice, e->stream));
        row0[n] = n, len[n] = 1, prior[n] = 0, sum_index[n] = 0, fin[n] = 1;
        ++n, ++n_finish;
    }
    if (n == 0) return TL_OK;  // LAST chunks that end no text: the pass has appended their K/V, nothing to pool
    TL_TRY(tl_rms_norm(mean ? e->shared.x_out : e->shared.h, e->final_norm, e->shared.xn, mean ? total : n, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
    TL_TRY(pool_rows(e->shared.xn, c.hidden_size, n, row0, len, fin, prior, sum_index, pooling, e->emb_sums, normalize, dim, e->emb_out, e->stream));
    if (n_finish == 0) return TL_OK;
    TL_HIP(hipMemcpyAsync(out_host, e->emb_out, (size_t)n_finish * dim * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    return TL_OK;
}

extern "C" int tl_engine_embed_packed(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, const int *finish,
                                      int pooling, int normalize, int dim, float *out_host) {
    TL_REQUIRE(e && slots && tokens && lens && finish, "engine_embed_packed: null argument");
    std::vector<PrefillSeq> seqs;
    int total = 0;
    TL_TRY(packed_seqs(e, n_seqs, slots, tokens, lens, nullptr, "engine_embed_packed", seqs, &total));
    bool finishes = false;
    for (int i = 0; i < n_seqs; ++i) finishes |= finish[i] != 0;
    TL_TRY(embed_args_check(e, pooling, dim, finishes, out_host));
    if (pooling == TL_POOL_MEAN) TL_TRY(embed_mean_check(e, seqs.data(), n_seqs));
    TL_TRY(prefill_pass(e, seqs.data(), n_seqs, tokens, total, true));
    return embed_pool(e, seqs.data(), n_seqs, finish, pooling, normalize, dim, out_host);
}

extern "C" int tl_engine_embed(tl_engine *e, int slot, const int32_t *tokens, int n, int finish, int pooling, int normalize, int dim,
                               float *out_host) {
    TL_REQUIRE(e && tokens, "engine_embed: null argument");
    TL_TRY(slot_check_feeds(e, slot));
    TL_TRY(embed_args_check(e, pooling, dim, finish != 0, out_host));
    const PrefillSeq seq{slot, e->table.slots[slot].ctx, 0, n};
    if (pooling == TL_POOL_MEAN) TL_TRY(embed_mean_check(e, &seq, 1));
    TL_TRY(prefill_impl(e, slot, tokens, n, 0));
    return embed_pool(e, &seq, 1, &finish, pooling, normalize, dim, out_host);
}

extern "C" int tl_engine_verify(tl_engine *e, int slot, const int32_t *tokens, int n, int32_t *out_ids) {
    TL_REQUIRE(e && out_ids, "engine_verify: null argument");
    TL_REQUIRE(n >= 1 && n <= VERIFY_MAX_LEN, "engine_verify: between 1 and 8 tokens per call (the paged decode kernel's query rows)");
    TL_TRY(slot_check_feeds(e, slot));
    TL_TRY(table_rc(e->settings.refuses_verify(slot)));
    TL_TRY(prefill_impl(e, slot, tokens, n, 2));
    TL_HIP(hipMemcpyAsync(out_ids, e->verify_ids, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    return TL_OK;
}

extern "C" int tl_engine_verify_sampled(tl_engine *e, int slot, const int32_t *tokens, int n, const void *draft_logits_dev, float draft_temperature,
                                        int draft_top_k, float draft_top_p, int32_t *out_ids, int *out_count) {
    TL_REQUIRE(e && tokens && out_ids && out_count, "engine_verify_sampled: null argument");
    TL_REQUIRE(n >= 1 && n <= VERIFY_MAX_LEN, "engine_verify_sampled: between 1 and 8 tokens per call (the paged decode kernel's query rows)");
    TL_REQUIRE(n == 1 || draft_logits_dev, "engine_verify_sampled: the rows the proposals were drawn from are missing");
    TL_REQUIRE(std::isfinite(draft_temperature) && draft_temperature >= 0.f, "engine_verify_sampled: the draft's temperature must be finite and >= 0");
    TL_TRY(slot_check_feeds(e, slot));
    TL_TRY(table_rc(e->settings.refuses_verify_sampled(slot)));
    TL_REQUIRE(e->cfg.vocab_size <= SMP_MAX_VOCAB, "engine_verify_sampled: vocabulary larger than the sampler's 524,288 tokens");
    using Rec = tl_engine::SpecRecord;
    if (!e->spec_rec) {
        TL_TRY(e->spec_mem.alloc(sizeof(Rec), "engine_verify_sampled: hipMalloc failed"));
        e->spec_rec = e->spec_mem.at<Rec>();
        e->stats.workspace_bytes += sizeof(Rec);
    }
    const int ctx = e->table.slots[slot].ctx;
    const SampleParams &sp = e->settings.slots[slot].smp;
    TL_TRY(prefill_impl(e, slot, tokens, n, 2));
    Rec r{};
    for (int i = 0; i < n; ++i) {
        r.proposal[i] = i + 1 < n ? tokens[i + 1] : -1;  // the last row is the bonus row
        r.t_temperature[i] = sp.temperature, r.t_top_k[i] = sp.top_k, r.t_top_p[i] = sp.top_p, r.seed[i] = sp.seed;
        r.d_temperature[i] = draft_temperature, r.d_top_k[i] = draft_top_k, r.d_top_p[i] = draft_top_p;
        r.position[i] = ctx + i + 1;
    }
    Rec *d = e->spec_rec;
    TL_HIP(hipMemcpyAsync(d, &r, offsetof(Rec, accept), hipMemcpyHostToDevice, e->stream));
    // (a bonus row's draft row is never read: with n == 1 the target's rows stand in for the missing pointer)
    TL_TRY(tl_spec_sample_rows(e->logits, draft_logits_dev ? draft_logits_dev : e->logits, n, e->cfg.vocab_size, d->proposal, d->t_temperature, d->t_top_k,
                               d->t_top_p, d->d_temperature, d->d_top_k, d->d_top_p, d->seed, d->position, d->accept, d->alt, e->stream));
    TL_HIP(hipMemcpyAsync(r.accept, d->accept, sizeof(r.accept) + sizeof(r.alt), hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    int a = 0;
    while (a < n - 1 && r.accept[a]) out_ids[a] = tokens[a + 1], ++a;
    out_ids[a] = r.alt[a];
    *out_count = a + 1;
    return TL_OK;
}

// ---- batched verification (include/tinyllm_engine.h "tl_engine_verify_batch"; the kernels are verify_attn.h) --------------------------
// the scratch of the pass, allocated by the first call
static int verify_alloc(tl_engine *e) {
    using V = VerifyLayout;
    tl_engine::VerifyScratch &v = e->vb;
    if (v.desc) return TL_OK;
    // the matmul workspace of 1 .. 64 rows, as tl_engine_create sizes the engine's own for its rows: only where that one is too small
    LayoutInputs in = layout_inputs(e);
    in.matmul_ws_need = matmul_ws_need(e, 1, VERIFY_BATCH_ROWS, 1, VERIFY_BATCH_ROWS, true);
    const VerifyLayout vl = verify_layout(e->cfg, in);
    TL_TRY(v.mem.alloc(vl.bytes, "engine_verify_batch: hipMalloc(scratch) failed"));
    char *m = v.mem.at();
    v.act = verify_act(m, vl);
    v.lin.xn = v.act.xn, v.lin.gu = piece_at<uint16_t>(m, vl[V::GU]), v.lin.tmp = piece_at<uint16_t>(m, vl[V::TMP]);
    v.lin.splitk_ws = vl.own_ws ? piece_at<void>(m, vl[V::MATMUL_WS]) : e->lin.splitk_ws;
    v.lin.splitk_ws_bytes = vl.own_ws ? in.matmul_ws_need : e->lin.splitk_ws_bytes;
    v.q = piece_at<uint16_t>(m, vl[V::Q]), v.logits = piece_at<uint16_t>(m, vl[V::LOGITS]), v.attn_ws_rows = in.verify_ws_rows;
    v.greedy = piece_at<int32_t>(m, vl[V::GREEDY]), v.results = piece_at<tl_verify_result>(m, vl[V::RESULTS]);
    v.desc = piece_at<int32_t>(m, vl[V::DESC]);
    e->stats.workspace_bytes += vl.bytes;
    return TL_OK;
}

// The checks of a batched verification and its sequences (pass_seqs holds what it shares with a packed pass).
// draft: NULL for the greedy call, else what tl_engine_verify_batch_sampled was given of the draft (its slots may sample).
struct VerifyDraft {
    const void *rows;  // [R, V] bf16 on the device; NULL: point proposals
    float temperature;
    int top_k;
    float top_p;
};
static int verify_seqs(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, bool commit, const VerifyDraft *draft,
                       std::vector<PrefillSeq> &seqs, int *total) {
    const tl_engine_config &c = e->cfg;
    const std::string w = draft ? "engine_verify_batch_sampled: " : "engine_verify_batch: ";
    TL_REQUIRE(n_seqs >= 1 && n_seqs <= VERIFY_BATCH_ROWS, w + "between 1 and 64 sequences per call");
    TL_REQUIRE(c.head_dim == VA_D, w + "head_dim 128");
    int rows = 0;
    for (int i = 0; i < n_seqs; ++i) {
        TL_REQUIRE(lens[i] >= 1 && lens[i] <= VERIFY_MAX_LEN, w + "between 1 and 8 tokens per sequence");
        rows += lens[i];
    }
    TL_REQUIRE(rows <= VERIFY_BATCH_ROWS, w + "the chunks together exceed 64 rows");
    bool moe = false;
    for (int l = 0; l < c.num_layers; ++l) moe |= e->is_moe(l);
    TL_REQUIRE(!moe || rows <= e->rows_cap, w + "a model with MoE layers takes at most max(max_batch, max_prefill_rows) rows (the experts' workspace)");
    // (a slot's refusal is met at its first appearance, ahead of "a slot appears twice" at its second, wherever it stands in the loop)
    if (draft) {
        TL_REQUIRE(std::isfinite(draft->temperature) && draft->temperature >= 0.f, w + "the draft's temperature must be finite and >= 0");
        TL_REQUIRE(c.vocab_size <= SMP_MAX_VOCAB, w + "vocabulary larger than the sampler's 524,288 tokens");
    }
    const auto per_seq = [&](int i) {
        return table_rc(draft ? e->settings.refuses_verify_batch_sampled(slots[i]) : e->settings.refuses_verify_batch(slots[i]));
    };
    return pass_seqs(e, n_seqs, slots, tokens, lens, commit, w, per_seq, [](int) { return (int)TL_OK; }, seqs, total);
}

// The pass over the `total` rows of the chunks in `seqs`, eager on the engine stream: pages reserved, tokens and descriptors uploaded in
// one copy, the rows embedded, then every layer on the shared-buffer decode route over the scratch's own buffers -- the projections
// through engine_linear with M = total (the sums of squares handed over where ProjResult says they were left, nothing weighted, no
// per-layer buffer), the attention stage of verify_attn.h in between -- the lm_head over all rows into the scratch's logits and the
// acceptance launches: the greedy pair, or with `draft` the sampling pair of verify_sample.h, which reads every slot's sampler parameters
// where SB_SAMPLE keeps them.  The slots end the pass as prefill_pass leaves them; e->logits and its owner stay as they were.
static int verify_pass(tl_engine *e, const PrefillSeq *seqs, int n_seqs, const int32_t *tokens, int total, const VerifyDraft *draft) {
    using V = tl_engine::VerifyScratch;
    const tl_engine_config &c = e->cfg;
    V &v = e->vb;
    const Act &b = v.act;
    TL_TRY(aql_drain(e));
    SlotEdits ed;
    Pokes pk;
    for (int i = 0; i < n_seqs; ++i) TL_TRY(table_rc(e->table.reserve(seqs[i].slot, seqs[i].start + seqs[i].len, ed)));
    TL_TRY(apply_edits(e, ed, pk));
    TL_TRY(poke(e, pk));
    constexpr int N = VERIFY_BATCH_ROWS;  // words per array of `desc`
    int32_t desc[V::DESC_ARRAYS * N] = {};
    int max_len = 1, max_ctx = 1;
    for (int i = 0; i < n_seqs; ++i) {
        const PrefillSeq &s = seqs[i];
        desc[V::SEQ_SLOT * N + i] = s.slot, desc[V::SEQ_ROW0 * N + i] = s.row0, desc[V::SEQ_LEN * N + i] = s.len;
        desc[V::SEQ_CTX * N + i] = s.start + s.len;
        for (int j = 0; j < s.len; ++j) {
            desc[V::TOKENS * N + s.row0 + j] = tokens[s.row0 + j];
            desc[V::ROW_SLOT * N + s.row0 + j] = s.slot, desc[V::ROW_POS * N + s.row0 + j] = s.start + j;
        }
        max_len = std::max(max_len, s.len), max_ctx = std::max(max_ctx, s.start + s.len);
    }
    TL_HIP(hipMemcpyAsync(v.desc, desc, sizeof(desc), hipMemcpyHostToDevice, e->stream));
    for (int i = 0; i < n_seqs; ++i)  // the chunks enter the history rows of slots armed for prompt lookup (lookup.h)
        TL_TRY(lookup_record_chunk(e, seqs[i].slot, v.arr(V::TOKENS) + seqs[i].row0, seqs[i].len, seqs[i].start));
    const VerifySplit sp = verify_pick_splits(n_seqs, c.num_heads, c.num_kv_heads, total, max_len, max_ctx, v.attn_ws_rows);

    TL_TRY(tl_quantized_embedding(v.arr(V::TOKENS), 0, e->embed.scales_dev, e->embed.biases_dev, e->embed.weight_dev, b.x_out, total, c.hidden_size,
                                  c.vocab_size, 128, 4, TL_BF16, e->stream));
    // the router's scratch for the duration of the pass: the RMSNorm rows, the unfused epilogues' rows and the matmul workspace of 64 rows
    // (the engine's own go back when the pass returns, however it returns: captured steps hold those addresses)
    struct CtxScratch {
        LinearScratch &ctx;
        const LinearScratch own;
        CtxScratch(LinearScratch &c_, const LinearScratch &pass) : ctx(c_), own(c_) { ctx = pass; }
        ~CtxScratch() { ctx = own; }
    } scratch(e->lin, v.lin);
    LinearCtx &ctx = e->lin;
    const bool kv8 = e->kv_format == TL_KV_FP8_E4M3;
    int x_ss = 0;  // partials per row in ss_x (0 = none): whatever the last writer of x left
    for (int l = 0; l < c.num_layers; ++l) {
        const tl_layer_weights &w = e->layers[l];
        ProjResult r;
        Proj p = proj(w.wqkv, b.x_out, b.qkv, total);
        p.pro = PRO_RMSNORM, p.norm_w = w.input_norm_dev, p.ss_in = x_ss ? b.ss_x_out : nullptr, p.ss_in_n = x_ss;
        TL_TRY(engine_linear(ctx, p));
        VerifyRowsArgs q{};
        q.qkv = b.qkv, q.q_norm_w = (const uint16_t *)w.q_norm_dev, q.k_norm_w = (const uint16_t *)w.k_norm_dev, q.q = v.q;
        q.key_pages = e->layer_k(l), q.value_pages = e->layer_v(l), q.key_scales = e->layer_ks(l), q.value_scales = e->layer_vs(l);
        q.block_table = e->block_table, q.row_slot = v.arr(V::ROW_SLOT), q.row_pos = v.arr(V::ROW_POS);
        q.page_size = c.page_size, q.max_pages = c.max_pages_per_seq, q.num_heads = c.num_heads, q.num_kv_heads = c.num_kv_heads;
        q.eps = c.rms_norm_eps, q.rope_base = c.rope_theta;
        VerifyAttnArgs a{};
        a.q = v.q, a.key_pages = q.key_pages, a.value_pages = q.value_pages, a.key_scales = q.key_scales, a.value_scales = q.value_scales;
        a.block_table = e->block_table, a.seq_slot = v.arr(V::SEQ_SLOT), a.seq_row0 = v.arr(V::SEQ_ROW0), a.seq_len = v.arr(V::SEQ_LEN);
        a.seq_ctx = v.arr(V::SEQ_CTX), a.out = b.attn, a.ws = b.attn_ws;
        a.page_size = c.page_size, a.max_pages = c.max_pages_per_seq, a.num_heads = c.num_heads, a.num_kv_heads = c.num_kv_heads;
        a.scale = 1.0f / sqrtf((float)c.head_dim);
        TL_TRY(launch_verify_attention(q, a, sp, total, n_seqs, kv8, e->stream));
        Proj po = proj(w.wo, b.attn, b.h, total);
        po.epi = EPI_RESIDUAL, po.residual = b.x_out, po.kind = 1;
        if (e->is_moe(l)) {  // wo + residual, then the MoE MLP as its own launches (no producer-side sums for the next layer)
            TL_TRY(engine_linear(ctx, po));
            TL_TRY(tl_rms_norm(b.h, w.post_norm_dev, b.xn, total, c.hidden_size, c.rms_norm_eps, TL_BF16, e->stream));
            TL_TRY(engine_moe_mlp(e, l, b.xn, b.h, b.x_out, total, nullptr));
            x_ss = 0;
            continue;
        }
        TL_REQUIRE(w.wgu.weight_dev != nullptr, "engine: a layer has neither a dense MLP nor experts (tl_engine_set_moe_layer)");
        po.ss_out = b.ss_h;
        TL_TRY(engine_linear(ctx, po, nullptr, &r));
        const int h_ss = r.ss_n;
        Proj pg = proj(w.wgu, b.h, b.act, total);
        pg.pro = PRO_RMSNORM, pg.norm_w = w.post_norm_dev, pg.epi = EPI_SWIGLU, pg.kind = 2, pg.ss_in = h_ss ? b.ss_h : nullptr, pg.ss_in_n = h_ss;
        TL_TRY(engine_linear(ctx, pg));
        Proj pd = proj(w.wdown, b.act, b.x_out, total);
        pd.epi = EPI_RESIDUAL, pd.residual = b.h, pd.kind = 3, pd.ss_out = b.ss_x_out;
        TL_TRY(engine_linear(ctx, pd, nullptr, &r));
        x_ss = r.ss_n;
    }
    Proj ph = proj(e->head(), b.x_out, v.logits, total);
    ph.pro = PRO_RMSNORM, ph.norm_w = e->final_norm, ph.kind = 4, ph.ss_in = x_ss ? b.ss_x_out : nullptr, ph.ss_in_n = x_ss;
    TL_TRY(engine_linear(ctx, ph));
    v.rows = total;
    if (draft) {
        const SlotSettings::Offsets &at = e->settings.at;
        VerifySampleArgs a{};
        a.target = v.logits, a.draft = (const uint16_t *)draft->rows, a.vocab = c.vocab_size, a.n_seqs = n_seqs;
        a.tokens = v.arr(V::TOKENS), a.seq_row0 = v.arr(V::SEQ_ROW0), a.seq_len = v.arr(V::SEQ_LEN), a.seq_ctx = v.arr(V::SEQ_CTX);
        a.seq_index = v.arr(V::SEQ_SLOT);
        a.temperature = e->sdev<float>(SB_SAMPLE, at.smp_temp), a.top_k = e->sdev<int32_t>(SB_SAMPLE, at.smp_topk);
        a.top_p = e->sdev<float>(SB_SAMPLE, at.smp_topp), a.seed = e->sdev<uint64_t>(SB_SAMPLE, at.smp_seed);
        a.d_temperature = draft->temperature, a.d_top_k = draft->top_k, a.d_top_p = draft->top_p;
        a.accept = v.accept, a.alt = v.alt;
        TL_TRY(launch_verify_sample(a, nullptr, total, v.results, e->stream));
    } else {
        TL_TRY(launch_verify_accept(v.logits, c.vocab_size, total, n_seqs, v.arr(V::TOKENS), v.arr(V::SEQ_ROW0), v.arr(V::SEQ_LEN), v.greedy, v.results,
                                    e->stream));
    }
    for (int i = 0; i < n_seqs; ++i) {
        e->table.appended(seqs[i].slot, tokens + seqs[i].row0, seqs[i].len);
        e->settings.appended(seqs[i].slot, false);  // a pending token that is appended is never fed again
        pk.emplace_back(e->context_lens + seqs[i].slot, seqs[i].start + seqs[i].len);
    }
    TL_TRY(poke(e, pk));
    e->stats.prefill_tokens += total;
    return TL_OK;
}

// the body of tl_engine_verify_batch and tl_engine_verify_batch_sampled: the checks, the pass, the results and the commit
static int verify_batch_call(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, int commit, const VerifyDraft *draft,
                             tl_verify_result *out) {
    TL_REQUIRE(e && slots && tokens && lens && out, draft ? "engine_verify_batch_sampled: null argument" : "engine_verify_batch: null argument");
    std::vector<PrefillSeq> seqs;
    int total = 0;
    TL_TRY(verify_seqs(e, n_seqs, slots, tokens, lens, commit != 0, draft, seqs, &total));
    TL_TRY(verify_alloc(e));
    if (draft && !e->vb.accept) {
        tl_engine::VerifyScratch &v = e->vb;
        const size_t bytes = 2 * (size_t)VERIFY_BATCH_ROWS * 4;
        TL_TRY(v.sampled_mem.alloc(bytes, "engine_verify_batch_sampled: hipMalloc failed"));
        v.accept = v.sampled_mem.at<int32_t>(), v.alt = v.accept + VERIFY_BATCH_ROWS;
        e->stats.workspace_bytes += bytes;
    }
    TL_TRY(verify_pass(e, seqs.data(), n_seqs, tokens, total, draft));
    TL_HIP(hipMemcpyAsync(out, e->vb.results, (size_t)n_seqs * sizeof(tl_verify_result), hipMemcpyDeviceToHost, e->stream));
    TL_HIP(hipStreamSynchronize(e->stream));
    if (!commit) return TL_OK;
    for (int i = 0; i < n_seqs; ++i) {  // (stream ordered behind the pass: no second synchronisation)
        const int a = out[i].count - 1;
        TL_REQUIRE(a >= 0 && a < lens[i], "engine_verify_batch: the acceptance launch left an impossible count");
        if (lens[i] - 1 - a > 0) TL_TRY(tl_engine_rewind(e, slots[i], lens[i] - 1 - a));
        TL_TRY(tl_engine_set_token(e, slots[i], out[i].ids[a]));
    }
    return TL_OK;
}

extern "C" int tl_engine_verify_batch(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, int commit,
                                      tl_verify_result *out) {
    return verify_batch_call(e, n_seqs, slots, tokens, lens, commit, nullptr, out);
}

extern "C" int tl_engine_verify_batch_sampled(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens,
                                              const void *draft_logits_dev, float draft_temperature, int draft_top_k, float draft_top_p, int commit,
                                              tl_verify_result *out) {
    const VerifyDraft draft{draft_logits_dev, draft_temperature, draft_top_k, draft_top_p};
    return verify_batch_call(e, n_seqs, slots, tokens, lens, commit, &draft, out);
}

extern "C" int tl_engine_copy_verify_logits(tl_engine *e, int row0, int rows, void *dst_dev) {
    TL_REQUIRE(e && dst_dev, "engine_copy_verify_logits: null argument");
    TL_REQUIRE(e->vb.rows > 0, "engine_copy_verify_logits: no batched verification has run yet");
    TL_REQUIRE(row0 >= 0 && rows >= 1 && row0 <= e->vb.rows - rows, "engine_copy_verify_logits: rows outside the last pass");
    TL_HIP(hipMemcpyAsync(dst_dev, e->vb.logits + (size_t)row0 * e->cfg.vocab_size, (size_t)rows * e->cfg.vocab_size * 2, hipMemcpyDeviceToDevice,
                          e->stream));
    return TL_OK;
}

// directory of this shared library: the device-only code objects of the AQL route lie next to it
static std::string library_dir() {
    Dl_info info{};
    if (dladdr((const void *)&library_dir, &info) == 0 || !info.dli_fname) return ".";
    const std::string path = info.dli_fname;
    const size_t slash = path.rfind('/');
    return slash == std::string::npos ? std::string(".") : path.substr(0, slash);
}

// everything the AQL queue holds has run: the stream may be used again (and the host may read what the steps wrote)
static int aql_drain(tl_engine *e) {
    if (e->aql_queue && e->aql_queue->busy()) {
        std::string why;
        if (!e->aql_queue->wait(30.0, why)) return fail(TL_ERR_HIP, "engine: " + why);
    }
    return TL_OK;
}

// ---- the parts of a decode step around enqueue_step (tl_engine_decode, tl_engine_profile_step, tl_engine_check_step)
// What the three entry points ask first: the batch, the device -- launches go to the CURRENT device's copy of a kernel, the AQL packets
// to the engine's own agent: both must be the engine's device -- and the stops the device has seen (a prefill's first token may have
// stopped its slot: the plan asks the table)
static int step_call_begin(tl_engine *e, int batch, const char *who) {
    TL_REQUIRE(batch > 0 && batch <= e->cfg.max_batch, std::string(who) + ": batch out of range");
    int dev_now = -1;
    TL_HIP(hipGetDevice(&dev_now));
    TL_REQUIRE(dev_now == e->device, "engine_decode: the current HIP device is not the device this engine was created on");
    return stop_reconcile(e);
}

// the features of a call's steps; input activations of slots [0, batch) for the first of them from their pending token ids, with its
// RoPE factors and sums of squares
static int step_inputs(tl_engine *e, int batch, StepFeatures *f) {
    const tl_engine_config &c = e->cfg;
    hipLaunchKernelGGL(embed_slots_kernel, dim3(batch), dim3(256), 0, e->stream, e->tokens, e->embed.weight_dev,
                       (const uint16_t *)e->embed.scales_dev, (const uint16_t *)e->embed.biases_dev, e->shared.x_out, c.hidden_size,
                       c.vocab_size, e->context_lens, e->rope_table, e->rope_cur, e->rope_positions, c.head_dim / 2, e->shared.ss_x_out);
    TL_CHECK_LAUNCH("engine embed");
    *f = step_features(e, 0, batch);
    if (f->stop) e->stop_dirty = true;  // (a replayed plan launches the stop check without passing through launch_stop)
    return TL_OK;
}

// what the replay route wants done before its answer is acted on (replay_route.h)
static int route_first(tl_engine *e, unsigned first) {
    if (first & DRAIN) TL_TRY(aql_drain(e));
    if (first & SYNC_STREAM) TL_HIP(hipStreamSynchronize(e->stream));
    if (first & FLUSH_PLANS) {
        e->plans.clear();
        e->stats.graph_cache_flushes++;
    }
    return TL_OK;
}
// every return of a call passes through ReplayCall::finish (an error return keeps its own status)
struct ReplayCallEnd {
    tl_engine *e;
    ReplayCall &call;
    ~ReplayCallEnd() { (void)route_first(e, call.finish()); }
};

// the pages of this step's token in every live slot of [0, batch), poked into the block table, and the step's split plan
static int prepare_step(tl_engine *e, int batch, AttnPlan *sp, ReplayCall &call) {
    SlotEdits &ed = e->step_edits;  // (reused: a step in which no slot crosses a page boundary allocates nothing)
    ed.clear();
    int max_ctx = 1;
    TL_TRY(table_rc(e->table.reserve_step(batch, ed, &max_ctx)));
    if (!ed.rows.empty()) {
        TL_TRY(route_first(e, call.pages_changed()));
        Pokes pk;
        TL_TRY(apply_edits(e, ed, pk));
        TL_TRY(poke(e, pk));
    }
    *sp = e->attn.plan(batch, max_ctx, e->kv_format == TL_KV_FP8_E4M3);
    return TL_OK;
}

// the launches of a step, eagerly on the stream (stamped and checked where `pc` says so)
static int eager_step(tl_engine *e, int batch, const AttnPlan &sp, const StepFeatures &f, ProfCtx *pc = nullptr) {
    TL_TRY(enqueue_step(e, batch, sp, f, pc));
    e->warmed = true;
    return TL_OK;
}

// the host mirrors after a step over slots [0, batch): every live slot holds one more token and has produced one more id
static void step_done(tl_engine *e, int batch, const StepFeatures &f) {
    e->table.step_done(batch);
    for (int b = 0; b < batch; ++b)
        if (e->slot_runs(b)) e->settings.pending_produced(b);
    e->stats.decode_steps++;
    if (f.lora) e->lora_steps++;
    e->logits_rows = batch, e->logits_slot = -1;
}

// One REAL eager step as a call of its own (tl_engine_profile_step, tl_engine_check_step), behind step_call_begin and step_inputs: state
// advances exactly like tl_engine_decode(e, batch, 1, 0)
static int one_eager_step(tl_engine *e, int batch, const StepFeatures &f, ProfCtx *pc, AttnPlan *sp) {
    ReplayCall call;  // (stays on the stream)
    TL_TRY(lookup_before_steps(e, batch, 1, nullptr));
    TL_TRY(prepare_step(e, batch, sp, call));
    TL_TRY(eager_step(e, batch, *sp, f, pc));
    step_done(e, batch, f);
    return stop_reconcile(e);
}

// a step of tl_engine_decode behind prepare_step and the route's answer for it: captured into a plan of the cache
static int capture_step(tl_engine *e, int batch, const AttnPlan &sp, const StepFeatures &f, const PlanKey &key, tl_engine::DecodePlan **out) {
    hipGraph_t graph = nullptr;
    TL_HIP(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_step(e, batch, sp, f);
    const hipError_t ce = hipStreamEndCapture(e->stream, &graph);
    if (rc != TL_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (ce != hipSuccess) return fail(TL_ERR_HIP, std::string("engine_decode: graph capture failed: ") + hipGetErrorString(ce));
    tl_engine::DecodePlan plan;
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    plan.exec.reset(exec);
    // the same nodes as packet templates (aql.h); a plan whose program cannot be built keeps the graph route
    if (ie == hipSuccess && program_wanted(e->aql_on, e->step_written_once, f)) {
        auto prog = std::make_unique<AqlProgram>();
        std::string why;
        if (aql_program_from_graph(*e->aql_rt, graph, e->stream, *prog, why) == 0) plan.program = std::move(prog);
    }
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess) return fail(TL_ERR_HIP, std::string("engine_decode: graph instantiate failed: ") + hipGetErrorString(ie));
    *out = e->plans.insert(key, std::move(plan));
    e->stats.graph_captures++;
    return TL_OK;
}

extern "C" int tl_engine_decode(tl_engine *e, int batch, int steps, int use_graph) {
    TL_REQUIRE(e, "engine_decode: null engine");
    TL_TRY(step_call_begin(e, batch, "engine_decode"));
    TL_REQUIRE(steps >= 0, "engine_decode: steps must be nonnegative");
    if (steps == 0) return TL_OK;
    std::vector<int> lookup_restart;  // (allocates nothing while no armed slot outruns the ring)
    struct LookupRestartEnd {  // however the call returns, behind the reconciliation at its end
        tl_engine *e;
        const std::vector<int> &slots;
        ~LookupRestartEnd() { lookup_steps_done(e, slots); }
    } const lookup_end{e, lookup_restart};
    TL_TRY(lookup_before_steps(e, batch, steps, &lookup_restart));
    StepFeatures f;
    TL_TRY(step_inputs(e, batch, &f));
    ReplayCall call;
    const ReplayCallEnd end{e, call};
    for (int s = 0; s < steps; ++s) {
        AttnPlan sp;
        TL_TRY(prepare_step(e, batch, &sp, call));
        const PlanKey key{batch, sp.key() | step_key_bits(f)};
        tl_engine::DecodePlan *plan = use_graph && e->warmed ? e->plans.find(key) : nullptr;
        const StepAnswer step = call.step(use_graph != 0, e->warmed, plan != nullptr, e->plans.full());
        TL_TRY(route_first(e, step.first));
        if (step.kind == StepKind::EAGER) {
            TL_TRY(eager_step(e, batch, sp, f));
        } else {
            if (step.kind == StepKind::CAPTURE) TL_TRY(capture_step(e, batch, sp, f, key, &plan));
            const ReplayAnswer go = call.replay(plan->program != nullptr, s + 1 == steps);
            TL_TRY(route_first(e, go.first));
            if (go.submit) {
                std::string why;
                if (!e->aql_queue->submit(*plan->program, e->aql_fences, go.first_packet, go.last_packet, why)) {
                    (void)route_first(e, call.finish());  // (ahead of the message below, which is the one the caller reads)
                    return fail(TL_ERR_HIP, "engine_decode: " + why);
                }
                e->stats.aql_steps++;
            } else {
                TL_HIP(hipGraphLaunch(plan->exec.get(), e->stream));
            }
            e->stats.graph_replays++;
        }
        step_done(e, batch, f);
    }
    TL_TRY(route_first(e, call.finish()));
    // a plan with an armed slot: the host mirrors follow the device before the call returns (synchronises, on every route)
    return stop_reconcile(e);
}

extern "C" int tl_engine_read_tokens(tl_engine *e, int slot, int count, int32_t *out) {
    TL_TRY(slot_check(e, slot, false));
    TL_REQUIRE(out && count >= 0 && count <= e->ring_cap, "engine_read_tokens: bad count");
    TL_REQUIRE(count <= e->table.slots[slot].produced, "engine_read_tokens: fewer ids have been produced");
    TL_HIP(hipStreamSynchronize(e->stream));
    std::vector<int32_t> ring(e->ring_cap);
    TL_HIP(hipMemcpy(ring.data(), e->ring + (size_t)slot * e->ring_cap, (size_t)e->ring_cap * 4, hipMemcpyDeviceToHost));
    const int produced = e->table.slots[slot].produced;
    for (int i = 0; i < count; ++i) out[i] = ring[(produced - count + i) % e->ring_cap];
    return TL_OK;
}

extern "C" const void *tl_engine_logits_dev(const tl_engine *e) { return e ? e->logits : nullptr; }
extern "C" int tl_engine_copy_logits(tl_engine *e, void *dst_dev, int rows) {
    TL_REQUIRE(e && dst_dev, "engine_copy_logits: null argument");
    TL_REQUIRE(rows > 0 && rows <= e->cfg.max_batch, "engine_copy_logits: rows out of range");
    TL_HIP(hipMemcpyAsync(dst_dev, e->logits, (size_t)rows * e->cfg.vocab_size * 2, hipMemcpyDeviceToDevice, e->stream));
    return TL_OK;
}
extern "C" int tl_engine_copy_processed_logits(tl_engine *e, void *dst_dev, int rows) {
    TL_REQUIRE(e && dst_dev, "engine_copy_processed_logits: null argument");
    TL_REQUIRE(rows > 0 && rows <= e->cfg.max_batch, "engine_copy_processed_logits: rows out of range");
    TL_REQUIRE(e->settings_mem[SB_PROCESS], "engine_copy_processed_logits: no slot of this engine has processed its logits yet");
    TL_HIP(hipMemcpyAsync(dst_dev, e->sdev<uint16_t>(SB_PROCESS, e->settings.at.pen_rows), (size_t)rows * e->cfg.vocab_size * 2, hipMemcpyDeviceToDevice, e->stream));
    return TL_OK;
}
extern "C" const int32_t *tl_engine_tokens_dev(const tl_engine *e) { return e ? e->tokens : nullptr; }

extern "C" int tl_engine_get_stats(const tl_engine *e, tl_engine_stats *out) {
    TL_REQUIRE(e && out, "engine_get_stats: null argument");
    *out = e->stats;
    page_stats(e->table, out);
    return TL_OK;
}

// bytes of a W4 matrix a decode step streams: the packed weights and one (scale, bias) pair per group of 128
static size_t w4_bytes(const tl_w4 &w) { return (size_t)w.rows * w.cols / 2 + (size_t)w.rows * (w.cols / 128) * 4; }

extern "C" size_t tl_engine_step_bytes(const tl_engine *e, int batch) {
    if (!e) return 0;
    const tl_engine_config &c = e->cfg;
    size_t total = 0;
    for (const auto &l : e->layers) total += w4_bytes(l.wqkv) + w4_bytes(l.wo) + w4_bytes(l.wgu) + w4_bytes(l.wdown);
    total += w4_bytes(e->head());
    // K and V rows of a cached token, all layers: 2 bytes per element, or (FP8 pages) one byte per element + a 4-byte scale per row
    const size_t kv_per_token = e->kv_format == TL_KV_FP8_E4M3 ? (size_t)2 * c.num_layers * c.num_kv_heads * (c.head_dim + 4)
                                                               : (size_t)2 * c.num_layers * c.num_kv_heads * c.head_dim * 2;
    for (int b = 0; b < batch && b < c.max_batch; ++b)
        if (e->slot_runs(b)) total += kv_per_token * (size_t)e->table.slots[b].ctx;
    return total;
}

// One REAL decode step (state advances exactly like tl_engine_decode(e, batch, 1, 0)) launched eagerly with
// in-kernel wall-clock stamps; see tl_step_profile in the header.
extern "C" int tl_engine_profile_step(tl_engine *e, int batch, tl_step_profile *out) {
    TL_REQUIRE(e && out, "engine_profile_step: null argument");
    TL_TRY(step_call_begin(e, batch, "engine_profile_step"));
    int rate_khz = 0;
    TL_HIP(hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, e->device));
    TL_REQUIRE(rate_khz > 0, "engine_profile_step: device reports no wall clock rate");
    TL_HIP(hipStreamSynchronize(e->stream));
    ProfCtx pc;
    if (!pc.alloc(e->cfg, batch, e->stream)) return fail(TL_ERR_HIP, "engine_profile_step: hipMalloc / memset of the stamp buffers failed");
    StepFeatures f;
    AttnPlan sp;
    int rc = step_inputs(e, batch, &f);
    if (rc == TL_OK) rc = one_eager_step(e, batch, f, &pc, &sp);
    if (rc != TL_OK) {
        (void)hipStreamSynchronize(e->stream);
        return rc;
    }
    std::vector<prof_t> pairs(pc.kinds.size() * 2);
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(pairs.data(), pc.pairs, pairs.size() * sizeof(prof_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(TL_ERR_HIP, std::string("engine_profile_step: ") + hipGetErrorString(he));

    *out = tl_step_profile{};
    out->clock_khz = rate_khz;
    out->n_splits = sp.n_splits;
    const double us_per_tick = 1e3 / (double)rate_khz;
    prof_t first = ~0ull, last = 0;
    for (size_t i = 0; i < pc.kinds.size(); ++i) {
        const prof_t t0 = pairs[2 * i], t1 = pairs[2 * i + 1];
        const double us = (t1 > t0 ? (double)(t1 - t0) : 0.0) * us_per_tick;
        first = std::min(first, t0);
        last = std::max(last, t1);
        out->kernel_us[pc.kinds[i]] += us;
        out->launches[pc.kinds[i]] += 1;
    }
    out->span_us = (last > first ? (double)(last - first) : 0.0) * us_per_tick;
    for (const auto &l : e->layers) {
        out->gemv_bytes[0] += w4_bytes(l.wqkv);
        out->gemv_bytes[1] += w4_bytes(l.wo);
        out->gemv_bytes[2] += w4_bytes(l.wgu);
        out->gemv_bytes[3] += w4_bytes(l.wdown);
    }
    out->gemv_bytes[4] = w4_bytes(e->head());
    return TL_OK;
}


// One REAL decode step, launched eagerly like tl_engine_profile_step, with the written-once checker behind every launch (header).
extern "C" int tl_engine_check_step(tl_engine *e, int batch, tl_step_check *out) {
    TL_REQUIRE(e && out, "engine_check_step: null argument");
    TL_TRY(step_call_begin(e, batch, "engine_check_step"));
    *out = tl_step_check{};
    out->first_launch = -1, out->first_kind = -1, out->first_region = -1, out->first_offset = -1;
    TL_TRY(aql_drain(e));
    TL_HIP(hipStreamSynchronize(e->stream));
    WrittenOnceCheck ck;
    ck.region[0] = e->arena.at(e->arena_act_off), ck.bytes[0] = (e->arena_bytes - e->arena_act_off) / 4 * 4;
    ck.region[1] = e->layer_act_mem.at(), ck.bytes[1] = e->layer_act_mem ? e->layer_act_bytes / 4 * 4 : 0;
    // the checker's buffers live in this frame; every return below has waited for the stream before they go
    struct StreamWait {
        hipStream_t s;
        ~StreamWait() { (void)hipStreamSynchronize(s); }
    };
    DeviceBlock shadow[2], written[2], report_mem;
    ProfCtx pc;
    const StreamWait wait_first{e->stream};
    const char *no_memory = "engine_check_step: hipMalloc of the shadow buffers failed";
    if (!pc.alloc(e->cfg, batch, e->stream)) return fail(TL_ERR_HIP, no_memory);
    TL_TRY(report_mem.alloc(8 * sizeof(unsigned long long), no_memory));
    ck.report = report_mem.at<unsigned long long>();
    for (int rg = 0; rg < 2; ++rg) {
        if (!ck.bytes[rg]) continue;
        TL_TRY(shadow[rg].alloc(ck.bytes[rg], no_memory));
        TL_TRY(written[rg].alloc(ck.bytes[rg] / 2, no_memory));
        ck.shadow[rg] = shadow[rg].at<uint32_t>(), ck.written[rg] = written[rg].at<uint8_t>();
    }
    bool ok = true;
    // the per-layer buffers start the step POISONED (every 16-bit and 32-bit pattern a NaN): a value read before this step wrote it
    // reaches the logits as NaN; the shared activations carry state between steps (x, its sums of squares) and keep their contents
    const unsigned long long report0[8] = {0, ~0ull, 0, 0, 0, 0, 0, 0};
    ok = hipMemcpyAsync(ck.report, report0, sizeof(report0), hipMemcpyHostToDevice, e->stream) == hipSuccess;
    if (ok && ck.bytes[1]) ok = hipMemsetAsync(ck.region[1], 0xff, ck.bytes[1], e->stream) == hipSuccess;
    if (!ok) return fail(TL_ERR_HIP, "engine_check_step: initialisation failed");
    StepFeatures f;
    TL_TRY(step_inputs(e, batch, &f));
    // the shadows = the regions as the step finds them; nothing written yet
    for (int rg = 0; rg < 2 && ok; ++rg)
        if (ck.bytes[rg]) ok = hipMemcpyAsync(ck.shadow[rg], ck.region[rg], ck.bytes[rg], hipMemcpyDeviceToDevice, e->stream) == hipSuccess &&
                               hipMemsetAsync(ck.written[rg], 0, ck.bytes[rg] / 2, e->stream) == hipSuccess;
    if (!ok) return fail(TL_ERR_HIP, "engine_check_step: shadow copy failed");
    AttnPlan sp;
    pc.check = &ck;
    TL_TRY(one_eager_step(e, batch, f, &pc, &sp));
    unsigned long long report[8] = {0};
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(report, ck.report, sizeof(report), hipMemcpyDeviceToHost);
    const std::vector<int> &kinds = pc.kinds;
    if (he != hipSuccess) return fail(TL_ERR_HIP, std::string("engine_check_step: ") + hipGetErrorString(he));
    out->launches = (int)kinds.size();
    out->written_once_plan = e->step_written_once ? 1 : 0;
    out->n_splits = sp.n_splits;
    out->double_writes = (long)report[0];
    out->elements_written = (long)report[3];
    if (report[0]) {
        out->first_launch = (int)report[1];
        out->first_kind = report[1] < kinds.size() ? kinds[report[1]] : -1;
        out->first_region = (int)report[2];
        out->first_offset = (long)report[4];
    }
    return TL_OK;
}

// ---- kernel-level entry points beside tl_decode_linear[_ex] (decode_linear.h): the prefill GEMM, the decode attention, the plans ----
// The prefill projection of large chunks on caller buffers (header): W4 -> bf16 expansion, then the plain bf16 GEMM of gemm8.h.
extern "C" int tl_prefill_weights_bf16(const tl_w4 *w, void *out_dev, void *stream) {
    TL_REQUIRE(w && out_dev, "prefill_weights_bf16: null argument");
    TL_TRY(check_w4(*w, w->rows, w->cols, "prefill_weights_bf16"));
    TL_REQUIRE(w->cols % 128 == 0, "prefill_weights_bf16: columns must be a multiple of the quantisation group (128)");
    if (dequant_w4_to_bf16(w->weight_dev, (const uint16_t *)w->scales_dev, (const uint16_t *)w->biases_dev, (uint16_t *)out_dev, w->rows, w->cols, (hipStream_t)stream) != 0)
        return fail(TL_ERR_HIP, "prefill_weights_bf16: launch failed");
    return TL_OK;
}
extern "C" int tl_prefill_matmul_bf16(const void *a_dev, const void *w_bf16_dev, void *out_dev, int M, int rows, int cols, int epilogue,
                                      const void *residual_dev, void *stream) {
    TL_REQUIRE(a_dev && w_bf16_dev && out_dev, "prefill_matmul_bf16: null argument");
    TL_REQUIRE(epilogue == EPI_STORE || epilogue == EPI_RESIDUAL || epilogue == EPI_SWIGLU, "prefill_matmul_bf16: epilogue is 0 (store), 1 (residual add) or 2 (SwiGLU over interleaved rows)");
    TL_REQUIRE(epilogue != EPI_RESIDUAL || residual_dev, "prefill_matmul_bf16: the residual epilogue needs the residual rows");
    TL_REQUIRE(gemm8_applicable(M, rows, cols), "prefill_matmul_bf16: needs M >= 1, an even number of weight rows and columns in whole 64-wide steps");
    Gemm8Args g{};
    g.a = (const uint16_t *)a_dev, g.w = (const uint16_t *)w_bf16_dev, g.out = (uint16_t *)out_dev, g.residual = (const uint16_t *)residual_dev;
    g.M = M, g.N = rows, g.K = cols;
    if (launch_gemm8_bf16(g, epilogue, (hipStream_t)stream) != 0) return fail(TL_ERR_UNSUPPORTED, "prefill_matmul_bf16: launch failed");
    TL_CHECK_LAUNCH("prefill_matmul_bf16");
    return TL_OK;
}

// (cos, sin) of each row's position = its context length, the same expression as rope_table_kernel
__global__ __launch_bounds__(64) void rope_rows_kernel(const int32_t *__restrict__ context_lens, float2 *__restrict__ rope_cur,
                                                       int half, float base) {
    const int b = blockIdx.x;
    const int pos = context_lens[b];
    for (int item = threadIdx.x; item < half; item += 64) {
        const float fp = -(float)item / (float)half;
        const float angle = (float)pos * exp2f(fp * log2f(base));
        float sn, cs;
        sincosf(angle, &sn, &cs);
        rope_cur[(long)b * half + item] = make_float2(cs, sn);
    }
}

extern "C" size_t tl_decode_attention_fused_workspace_bytes(int batch, int num_heads, int head_dim) {
    if (batch <= 0 || num_heads <= 0 || head_dim <= 0) return 0;
    return align_up((size_t)batch * (head_dim / 2) * sizeof(float2), 256) + attn_partials_bytes(batch, num_heads, 256, head_dim);  // (TL_ATTN_MAX_SPLITS <= 256)
}

static int decode_attention_fused_impl(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev,
                                       float *key_scales_dev, void *value_pages_dev, float *value_scales_dev,
                                       const int32_t *block_table_dev, const int32_t *context_lens_dev, void *out_dev, int batch,
                                       int num_heads, int num_kv_heads, int head_dim, int page_size, int max_pages, float rope_theta,
                                       float eps, int max_context, void *workspace_dev, size_t workspace_bytes, void *stream,
                                       tl_attention_info *info) {
    TL_REQUIRE(qkv_dev && q_norm_dev && k_norm_dev && key_pages_dev && value_pages_dev && block_table_dev && context_lens_dev &&
                   out_dev, "decode_attention_fused: null pointer");
    TL_REQUIRE(batch >= 1 && batch <= 256, "decode_attention_fused: between 1 and 256 sequences");
    TL_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0,
               "decode_attention_fused: num_heads must be divisible by num_kv_heads");
    TL_REQUIRE(head_dim == 32 || head_dim == 64 || head_dim == 128, "decode_attention_fused: head_dim must be 32, 64 or 128");
    TL_REQUIRE(page_size > 0 && max_pages > 0 && max_context >= 0, "decode_attention_fused: bad page geometry");
    const size_t need = tl_decode_attention_fused_workspace_bytes(batch, num_heads, head_dim);
    TL_REQUIRE(workspace_dev && workspace_bytes >= need, "decode_attention_fused: workspace is missing or too small");
    AttnCtx ctx;
    ctx.geometry = AttnGeometry{num_heads, num_kv_heads, head_dim, page_size, max_pages};
    ctx.eps = eps, ctx.rope_theta = rope_theta, ctx.stream = (hipStream_t)stream;
    ctx.block_table = block_table_dev, ctx.context_lens = context_lens_dev, ctx.rope_cur = (const float2 *)workspace_dev;
    const size_t rc_bytes = align_up((size_t)batch * (head_dim / 2) * sizeof(float2), 256);
    ctx.ws_bytes = workspace_bytes - rc_bytes;
    ctx.knobs.read_env();
    hipLaunchKernelGGL(rope_rows_kernel, dim3(batch), dim3(64), 0, ctx.stream, context_lens_dev, (float2 *)workspace_dev, head_dim / 2, rope_theta);
    TL_CHECK_LAUNCH("decode_attention_fused rope");
    const AttnPlan sp = ctx.plan(batch, std::max(1, max_context + 1), key_scales_dev != nullptr);
    AttnCall at{};
    at.qkv = (const uint16_t *)qkv_dev, at.q_norm = q_norm_dev, at.k_norm = k_norm_dev, at.out = (uint16_t *)out_dev;
    at.key_pages = (uint16_t *)key_pages_dev, at.value_pages = (uint16_t *)value_pages_dev, at.key_scales = key_scales_dev, at.value_scales = value_scales_dev;
    at.ws = (float *)((char *)workspace_dev + rc_bytes);
    const int rc = launch_decode_attention(ctx, sp, at, batch, nullptr);
    if (info) {
        info->n_splits = sp.n_splits;
        info->tokens_per_split = sp.tokens_per_split;
        info->heads_per_workgroup = sp.rq;
        info->launches = rc == TL_OK ? sp.launches() : 0;
    }
    return rc;
}

extern "C" int tl_decode_attention_fused(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev,
                                         void *key_pages_dev, void *value_pages_dev, const int32_t *block_table_dev,
                                         const int32_t *context_lens_dev, void *out_dev, int batch, int num_heads,
                                         int num_kv_heads, int head_dim, int page_size, int max_pages, float rope_theta,
                                         float eps, int max_context, void *workspace_dev, size_t workspace_bytes,
                                         void *stream, tl_attention_info *info) {
    return decode_attention_fused_impl(qkv_dev, q_norm_dev, k_norm_dev, key_pages_dev, nullptr, value_pages_dev, nullptr, block_table_dev,
                                       context_lens_dev, out_dev, batch, num_heads, num_kv_heads, head_dim, page_size, max_pages, rope_theta,
                                       eps, max_context, workspace_dev, workspace_bytes, stream, info);
}

extern "C" int tl_decode_attention_fused_fp8(const void *qkv_dev, const void *q_norm_dev, const void *k_norm_dev, void *key_pages_dev,
                                             float *key_scales_dev, void *value_pages_dev, float *value_scales_dev,
                                             const int32_t *block_table_dev, const int32_t *context_lens_dev, void *out_dev, int batch,
                                             int num_heads, int num_kv_heads, int head_dim, int page_size, int max_pages,
                                             float rope_theta, float eps, int max_context, void *workspace_dev, size_t workspace_bytes,
                                             void *stream, tl_attention_info *info) {
    TL_REQUIRE(key_scales_dev && value_scales_dev, "decode_attention_fused_fp8: null scale pointer");
    TL_REQUIRE(head_dim == 128, "decode_attention_fused_fp8: FP8 pages need head_dim 128");
    return decode_attention_fused_impl(qkv_dev, q_norm_dev, k_norm_dev, key_pages_dev, key_scales_dev, value_pages_dev, value_scales_dev,
                                       block_table_dev, context_lens_dev, out_dev, batch, num_heads, num_kv_heads, head_dim, page_size,
                                       max_pages, rope_theta, eps, max_context, workspace_dev, workspace_bytes, stream, info);
}

// ---- host-only: the plans the decode path would pick (no device, no launch): what the CPU tests and a binding's dry run read -------
extern "C" int tl_decode_gemv_plan(int M, int rows, int cols, int *out5) {
    if (!out5 || M < 1 || rows <= 0 || cols <= 0) return 0;
    const Qmv3Plan pl = qmv3_plan(M, cols, rows);
    out5[0] = pl.MR, out5[1] = pl.KS, out5[2] = pl.CW, out5[3] = pl.LM, out5[4] = pl.blocks;
    return pl.ok ? 1 : 0;
}
extern "C" int tl_decode_gemv_variant_compiled(int MR, int KS, int CW, int LM) { return qmv3_has_variant(MR, KS, CW, LM) ? 1 : 0; }
extern "C" int tl_decode_batched_plan(int M, int rows, int cols, int *out6) {
    if (!out6 || M < 1 || rows <= 0 || cols <= 0) return 0;
    const Qmm6Plan pl = qmm6_plan(M, cols, rows, false, qmm3_num_cus());
    out6[0] = pl.MB, out6[1] = pl.GPW, out6[2] = pl.NSETS, out6[3] = pl.row_blocks, out6[4] = pl.wgs, out6[5] = pl.tiles_per_wg;
    return pl.ok ? 1 : 0;
}
extern "C" int tl_decode_batched_variant_compiled(int MB, int GPW) { return qmm6_has_variant(MB, GPW) ? 1 : 0; }
extern "C" int tl_decode_streaming_plan(int M, int rows, int cols, int *out4) {
    if (!out4 || M < 1 || rows <= 0 || cols <= 0) return 0;
    const Qmm7Plan pl = qmm7_plan(M, cols, rows, qmm3_num_cus());
    out4[0] = pl.MB, out4[1] = pl.T, out4[2] = pl.GPW, out4[3] = pl.wgs;
    return pl.ok ? 1 : 0;
}
extern "C" int tl_decode_streaming_variant_compiled(int T, int GPW) { return qmm7_has_variant(T, GPW) ? 1 : 0; }
extern "C" int tl_decode_attention_plan(int batch, int max_context, int num_heads, int num_kv_heads, int *out3) {
    if (!out3 || batch < 1 || max_context < 0 || num_heads <= 0 || num_kv_heads <= 0 || num_heads % num_kv_heads != 0) return 0;
    AttnCtx ctx;
    ctx.geometry = AttnGeometry{num_heads, num_kv_heads, 128, 128, 1};  // the plan of the Qwen3 head size on 128-token pages
    ctx.knobs.read_env();
    const AttnPlan sp = ctx.plan(batch, std::max(1, max_context + 1), false);
    out3[0] = sp.n_splits, out3[1] = sp.tokens_per_split, out3[2] = sp.rq;
    return 1;
}

extern "C" int tl_kv_copy_rows(const tl_kv_pool_desc *pools_dev, int n_pools, int heads, int page_size, int from_page, int to_page,
                               int rows, void *stream) {
    return kv_copy_rows(pools_dev, n_pools, heads, page_size, from_page, to_page, rows, (hipStream_t)stream);
}

extern "C" size_t tl_kv_page_record_bytes(const tl_kv_pool_desc *pools_host, int n_pools, int heads, int page_size) {
    return kv_page_record_bytes(pools_host, n_pools, heads, page_size);
}
extern "C" int tl_kv_gather_pages(const tl_kv_pool_desc *pools_dev, const size_t *record_offsets_dev, int n_pools, int heads, int page_size,
                                  const int32_t *page_ids_dev, int n_pages, int tail_rows, void *staging_dev, size_t record_bytes, void *stream) {
    return kv_swap_pages<true>(pools_dev, record_offsets_dev, n_pools, heads, page_size, page_ids_dev, n_pages, tail_rows, staging_dev, record_bytes,
                               (hipStream_t)stream);
}
extern "C" int tl_kv_scatter_pages(const tl_kv_pool_desc *pools_dev, const size_t *record_offsets_dev, int n_pools, int heads, int page_size,
                                   const int32_t *page_ids_dev, int n_pages, int tail_rows, const void *staging_dev, size_t record_bytes, void *stream) {
    return kv_swap_pages<false>(pools_dev, record_offsets_dev, n_pools, heads, page_size, page_ids_dev, n_pages, tail_rows, (void *)staging_dev,
                                record_bytes, (hipStream_t)stream);
}
