// The replay route of tl_engine_decode (host only: no HIP, nothing of the project but slot_settings.h for StepFeatures;
// tests/replay_route_check.cpp compiles it with plain g++ and drives it over a fake device): which captured plan a step is, whether the
// plan may ride the engine's own AQL queue, and who owns the work of a call -- the HIP stream or that queue.  Two rules (DESIGN.md
// section 5):
//   * whatever must land on the STREAM between two steps of a call first drains the queue; every call ends drained;
//   * a program is built iff the route is on, the step was written once and graph_only_reason is null.
// The engine executes what ReplayCall answers; it decides nothing of this itself.
#pragma once

#include <cstddef>
#include <map>
#include <string>
#include <utility>

#include "slot_settings.h"

namespace tl {

// ---- which plan a step is ------------------------------------------------------------------------------------------------------------
// the bits a decode plan's key carries above its split plan (tl_engine_decode): with all clear the step is the greedy program
inline long step_key_bits(const StepFeatures &f) {
    // bit 62: the step ends with the sampling twin of step_end_kernel, bit 61: with the logprob twin (step_end.h)
    return (f.samples ? (1L << 62) : 0L) | (f.logprobs ? (1L << 61) : 0L) |
           // bit 60: the processing launch (logit_process.h) stands between the lm_head and the step end
           // bit 59: ... in its regex mode (grammar.h); bit 58: in its stack mode (grammar_stack.h)
           (f.processes ? (1L << 60) : 0L) | (f.grammar ? (1L << 59) : 0L) | (f.stack_grammar ? (1L << 58) : 0L) |
           // bit 57: the truncation launch (truncate.h) stands ahead of the step end and the Mirostat update behind it
           // bit 56: ... and a slot has Mirostat on (the plan keeps the hipGraphLaunch route)
           (f.truncates ? (1L << 57) : 0L) | (f.mirostat ? (1L << 56) : 0L) |
           // bit 55: a slot carries a LoRA adapter: the adapter plan (lora.h; hipGraphLaunch)
           (f.lora ? (1L << 55) : 0L) |
           // bit 54: a slot is armed with stop conditions: the stop launch (stop.h) stands last (hipGraphLaunch)
           (f.stop ? (1L << 54) : 0L) |
           // bit 53: a slot has DRY or the n-gram ban on: the match and apply launches (dry.h) stand behind the processing launch (hipGraphLaunch)
           (f.dry ? (1L << 53) : 0L);
}
// Why a plan with these features never becomes an AQL program (null: it may), the one sentence tl_engine_replay_route reports: bits 53,
// 54, 55 and 56 above, the stop launch first
inline const char *graph_only_reason(const StepFeatures &f) {
    if (f.stop) return "a slot is armed with stop conditions (the stop launch reads the token the step end stored and writes the live word)";
    if (f.lora) return "a slot with a LoRA adapter is live (the adapter plan hands over in shared buffers)";
    if (f.mirostat) return "a Mirostat slot is live (the update launch reads the token the step end stored)";
    if (f.dry) return "a slot has DRY or the n-gram ban on (the apply launch writes the processed rows a second time)";
    return nullptr;
}
// A captured step also becomes a program of AQL packets iff the engine has the route, every hand-over of the step as it was just enqueued
// is written once (no launch needs a boundary with cache maintenance) and no feature keeps the graph.  (A plan whose program cannot be
// built -- a kernel outside the device-only code objects -- keeps the graph route all the same.)
inline bool program_wanted(bool aql_on, bool written_once, const StepFeatures &f) { return aql_on && written_once && !graph_only_reason(f); }
// what tl_engine_replay_route reports: `live` are the features of every live slot (a plan of theirs that keeps hipGraphLaunch on an
// engine whose other plans ride the route is named by its reason)
inline std::string replay_route_text(bool aql_on, const std::string &aql_why, const StepFeatures &live) {
    if (!aql_on) return "hipgraph" + (aql_why.empty() ? std::string() : ": " + aql_why);
    const char *why = graph_only_reason(live);
    return why ? std::string("hipgraph: ") + why : std::string("aql");
}

// ---- the captured plans ----------------------------------------------------------------------------------------------------------------
struct PlanKey {
    int batch;
    long bits;  // AttnPlan::key() | step_key_bits(features)
    bool operator<(const PlanKey &o) const { return batch != o.batch ? batch < o.batch : bits < o.bits; }
};
// The split plan (and with it the key) changes every 64 * n_splits tokens of context: a long run would keep one ~220-node executable
// graph per plan and row bucket for ever.  Plans are visited in order of growing context, so when the cache is full the old ones are
// dead: the caller drops them all (a live plan is re-captured once, ~0.3 ms).  `Plan` is move-only and releases what it holds itself.
template <class Plan>
class PlanCache {
    std::map<PlanKey, Plan> plans;

  public:
    static constexpr size_t CAPACITY = 48;
    Plan *find(const PlanKey &key) {
        auto it = plans.find(key);
        return it == plans.end() ? nullptr : &it->second;
    }
    Plan *insert(const PlanKey &key, Plan &&plan) { return &plans.insert_or_assign(key, std::move(plan)).first->second; }
    void clear() { plans.clear(); }
    bool empty() const { return plans.empty(); }
    size_t size() const { return plans.size(); }
    bool full() const { return plans.size() >= CAPACITY; }
};

// ---- one decode call ---------------------------------------------------------------------------------------------------------------------
// What must happen before the answer may be acted on, in this order.  A DRAIN that was asked for counts as done whether or not it
// succeeded: the error goes to the caller, nobody waits for the queue a second time.
enum RouteFirst : unsigned {
    DRAIN = 1,        // wait until everything the AQL queue holds has run
    SYNC_STREAM = 2,  // wait until everything the stream holds has run
    FLUSH_PLANS = 4,  // clear the plan cache (and count the flush)
};
enum class StepKind { EAGER, CAPTURE, REPLAY };
struct StepAnswer {
    unsigned first;
    StepKind kind;
};
struct ReplayAnswer {
    unsigned first;
    bool submit;            // the plan's program goes to the queue (else: hipGraphLaunch on the stream)
    bool first_packet;      // ... as the first of a run: the queue was idle (its first packet acquires what the stream wrote)
    bool last_packet;       // ... as the last of the call (its last packet releases to the host)
};

// The state of one tl_engine_decode call: the call's steps so far are in flight on the AQL queue (the stream is idle and must stay so
// until they are drained), or everything stands on the stream.
class ReplayCall {
    bool queued = false;
    unsigned leave_queue() {
        const unsigned first = queued ? DRAIN : 0u;
        queued = false;
        return first;
    }

  public:
    bool on_queue() const { return queued; }
    // a step's new page ids are poked into the block table: a stream launch that must land between the steps
    unsigned pages_changed() { return leave_queue(); }
    // the step behind prepare_step.  `cached`: the cache holds the step's plan; `cache_full`: it holds CAPACITY plans
    StepAnswer step(bool use_graph, bool warmed, bool cached, bool cache_full) {
        if (!use_graph || !warmed) return {leave_queue(), StepKind::EAGER};  // (an engine's first step is never captured)
        if (cached) return {0u, StepKind::REPLAY};
        // a capture records stream launches; the executable graphs of a full cache go only when nothing on the stream can still run them
        const unsigned first = leave_queue();
        return {first | (cache_full ? SYNC_STREAM | FLUSH_PLANS : 0u), StepKind::CAPTURE};
    }
    // the replay of the step's plan (cached or just captured)
    ReplayAnswer replay(bool has_program, bool last_step) {
        if (!has_program) return {leave_queue(), false, false, false};
        // hand-over stream -> queue: everything enqueued so far (embedding gather, pokes, earlier steps) has run
        const bool hand_over = !queued;
        queued = true;
        return {hand_over ? SYNC_STREAM : 0u, true, hand_over, last_step};
    }
    // the end of the call and every error return: the queue is not the stream, and what follows the call (reads, prefills, the next
    // call's embedding gather) is stream-ordered
    unsigned finish() { return leave_queue(); }
};

}  // namespace tl
