// The replay route of tl_engine_decode alone (csrc/replay_route.h), over a fake device.
//
//   replay_route_check check   a seeded walk of decode calls -- batch, steps, feature set, page crossings, use_graph, route on / off, written
//                              once or not drawn at random; refused reservations, failed submits, drains, captures and refused programs
//                              injected -- through the loop tl_engine_decode runs, with a stream that is idle after a sync, a queue that is busy
//                              from a submit until a drain and a plan cache in the device's place.  The properties below are stated here,
//                              independently of the header's rules, and checked at every action.
//   replay_route_check trace   reads scenarios from stdin (tests/test_replay_route_cpu.py writes them from tests/golden/replay_routes.json,
//                              recorded on the GPU before the header existed) and prints, per call, the counters it moved and the route text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "attn_plan.h"
#include "replay_route.h"

using namespace tl;

static long g_checks = 0, g_calls = 0, g_steps = 0;
static void require(bool ok, const char *what) {
    ++g_checks;
    if (ok) return;
    std::printf("FAILED call %ld step %ld: %s\n", g_calls, g_steps, what);
    std::exit(1);
}

static StepFeatures features_of(unsigned mask) {  // bit order: FEATURES of tests/test_replay_route_cpu.py
    StepFeatures f;
    bool *const field[] = {&f.samples, &f.logprobs, &f.processes, &f.grammar, &f.stack_grammar, &f.truncates, &f.mirostat, &f.lora, &f.stop, &f.dry};
    for (int i = 0; i < 10; ++i) *field[i] = (mask >> i) & 1;
    return f;
}

// a captured plan of the fake: move-only like the engine's; alive() counts the plans that exist
struct FakePlan {
    static long &alive() {
        static long n = 0;
        return n;
    }
    struct Gone {
        void operator()(int *p) const {
            --alive();
            delete p;
        }
    };
    std::unique_ptr<int, Gone> token{(++alive(), new int(0))};
    bool has_program = false, graph_only = false;
};

enum Rc { OK = 0, REFUSED, DRAIN_FAILED, CAPTURE_FAILED, SUBMIT_FAILED, RC_COUNT };

// The device's place: a stream that is idle after a sync, a queue that is busy from a submit until a drain, the plan cache, the counters
struct Fake {
    bool aql_on = true, written_once = true, warmed = false;
    bool stream_idle = true, queue_busy = false, last_was_sync = false;
    bool fail_next_drain = false, drain_failed = false;
    PlanCache<FakePlan> cache;
    std::set<std::pair<int, long>> shadow;  // the keys captured since the last flush, kept by the check itself
    long decode_steps = 0, graph_captures = 0, graph_replays = 0, aql_steps = 0, graph_cache_flushes = 0;
    long misses = 0, lost_misses = 0, refused_programs = 0;  // lookups that found no plan; those whose capture failed (no plan, no step)
    int call_steps = 0, call_step = 0;  // the call in progress

    void stream_action(const char *what) {  // poke, capture, graph launch, eager step
        require(!queue_busy, what);
        stream_idle = false, last_was_sync = false;
    }
    int drain() {
        last_was_sync = false;
        if (fail_next_drain && queue_busy) {
            fail_next_drain = false, drain_failed = true;
            return DRAIN_FAILED;  // (the queue stays busy: the wait ran out)
        }
        queue_busy = false;
        return OK;
    }
    void sync() { stream_idle = true, last_was_sync = true; }
    void flush() {
        require(cache.full(), "a flush of a cache that is not full");
        require(stream_idle && last_was_sync, "a flush without a stream sync directly before it");
        require(!queue_busy, "a flush while the queue is busy");
        cache.clear();
        require(FakePlan::alive() == 0, "a cleared cache keeps plans alive");
        shadow.clear();
        graph_cache_flushes++;
        last_was_sync = false;
    }
    int first(unsigned flags) {  // engine.hip route_first
        if (flags & DRAIN)
            if (drain() != OK) return DRAIN_FAILED;
        if (flags & SYNC_STREAM) sync();
        if (flags & FLUSH_PLANS) flush();
        return OK;
    }
    bool submit(const FakePlan &plan, bool first_packet, bool last_packet, bool fails) {
        require(plan.has_program, "a submit of a plan without a program");
        require(!plan.graph_only, "a plan with a graph-only reason was submitted");
        require(first_packet == !queue_busy, "`first` must be set exactly when the queue was idle");
        if (first_packet) require(last_was_sync && stream_idle, "the first submit of a run must directly follow a stream sync");
        require(last_packet == (call_step + 1 == call_steps), "`last` must be set on the call's final step and on no other");
        last_was_sync = false;
        if (fails) return false;
        queue_busy = true;
        return true;
    }
};

struct StepIn {
    long plan_key = 0;  // AttnPlan::key()
    bool new_page = false, refuse_reservation = false, fail_capture = false, refuse_program = false, fail_submit = false;
};

struct CallEnd {
    Fake &d;
    ReplayCall &call;
    ~CallEnd() { (void)d.first(call.finish()); }
};

// tl_engine_decode's loop over the fake
static int fake_decode(Fake &d, int batch, const StepFeatures &f, bool use_graph, const std::vector<StepIn> &steps) {
    if (steps.empty()) return OK;
    d.call_steps = (int)steps.size();
    d.stream_action("the embedding gather of a call while the queue is busy");
    ReplayCall call;
    const CallEnd end{d, call};
    for (int s = 0; s < (int)steps.size(); ++s) {
        const StepIn &in = steps[s];
        d.call_step = s, ++g_steps;
        // prepare_step
        if (in.refuse_reservation) return REFUSED;
        if (in.new_page) {
            if (d.first(call.pages_changed()) != OK) return DRAIN_FAILED;
            d.stream_action("a block-table poke while the queue is busy");
        }
        const PlanKey key{batch, in.plan_key | step_key_bits(f)};
        FakePlan *plan = use_graph && d.warmed ? d.cache.find(key) : nullptr;
        if (use_graph && d.warmed) {
            require((plan != nullptr) == (d.shadow.count({key.batch, key.bits}) == 1), "the cache and the keys captured since the last flush differ");
            if (!plan) d.misses++;
        }
        const StepAnswer step = call.step(use_graph, d.warmed, plan != nullptr, d.cache.full());
        require(step.kind == (!use_graph || !d.warmed ? StepKind::EAGER : plan ? StepKind::REPLAY : StepKind::CAPTURE), "the wrong kind of step");
        if (d.first(step.first) != OK) {
            if (step.kind == StepKind::CAPTURE) d.lost_misses++;
            return DRAIN_FAILED;
        }
        if (step.kind == StepKind::EAGER) {
            d.stream_action("an eager step while the queue is busy");
            d.warmed = true;
        } else {
            if (step.kind == StepKind::CAPTURE) {
                d.stream_action("a capture while the queue is busy");
                require(!d.cache.full(), "a capture into a full cache");
                if (in.fail_capture) {
                    d.lost_misses++;
                    return CAPTURE_FAILED;
                }
                FakePlan fresh;
                fresh.graph_only = f.stop || f.lora || f.mirostat || f.dry;  // (stated here, not asked of the header)
                const bool wanted = program_wanted(d.aql_on, d.written_once, f);
                require(wanted == (d.aql_on && d.written_once && !f.stop && !f.lora && !f.mirostat && !f.dry), "program_wanted is not the rule");
                fresh.has_program = wanted && !in.refuse_program;
                if (wanted && in.refuse_program) d.refused_programs++;
                plan = d.cache.insert(key, std::move(fresh));
                d.shadow.insert({key.batch, key.bits});
                d.graph_captures++;
                require(d.cache.size() <= PlanCache<FakePlan>::CAPACITY && d.cache.size() <= 48, "the cache holds more than 48 plans");
                require(d.cache.size() == d.shadow.size() && (long)d.cache.size() == FakePlan::alive(), "plans leaked or lost");
            }
            require(!plan->has_program || !plan->graph_only, "a plan with a graph-only reason has a program");
            const ReplayAnswer go = call.replay(plan->has_program, s + 1 == (int)steps.size());
            require(go.submit == plan->has_program, "a plan rides the queue exactly when it has a program");
            if (d.first(go.first) != OK) return DRAIN_FAILED;
            if (go.submit) {
                if (!d.submit(*plan, go.first_packet, go.last_packet, in.fail_submit)) {
                    (void)d.first(call.finish());
                    return SUBMIT_FAILED;
                }
                d.aql_steps++;
            } else {
                d.stream_action("hipGraphLaunch while the queue is busy");
            }
            d.graph_replays++;
        }
        d.decode_steps++;
        require(call.on_queue() == d.queue_busy, "the record and the queue disagree about who owns the call");
    }
    return d.first(call.finish());
}

static int run_check(unsigned seed, long calls) {
    // step_key_bits: one bit per feature, all above AttnPlan::key()
    {
        std::set<long> seen;
        for (unsigned m = 0; m < 1024; ++m) {
            const long bits = step_key_bits(features_of(m));
            require(seen.insert(bits).second, "step_key_bits gives two feature sets the same bits");
            require((bits & ((1L << 53) - 1)) == 0 && bits >= 0, "step_key_bits touches the bits of AttnPlan::key() (or the sign)");
            for (int i = 0; i < 10; ++i)
                if (!((m >> i) & 1)) require(step_key_bits(features_of(m | (1u << i))) != bits, "a feature does not move the key");
        }
        AttnPlan widest;
        widest.rq = AD_RQ, widest.n_splits = 256, widest.tokens_per_split = 1 << 23;
        require(widest.key() < (1L << 53), "AttnPlan::key() reaches bit 53");
        StepFeatures none;
        require(replay_route_text(true, "", none) == "aql" && replay_route_text(false, "", none) == "hipgraph" &&
                    replay_route_text(false, "no agent", features_of(1u << 8)) == "hipgraph: no agent",
                "the route text of an engine without a graph-only slot");
        for (int i : {6, 7, 8, 9}) {  // Mirostat, LoRA, stop, DRY
            const char *why = graph_only_reason(features_of(1u << i));
            require(why != nullptr && !program_wanted(true, true, features_of(1u << i)), "a Mirostat, LoRA, stop-armed or DRY plan would get a program");
            require(replay_route_text(true, "", features_of(1u << i)) == std::string("hipgraph: ") + why, "the route text names the reason");
        }
    }
    std::mt19937 rng(seed);
    auto chance = [&](int percent) { return (int)(rng() % 100) < percent; };
    long flushes = 0, ended[RC_COUNT] = {0}, submitted = 0, refused_programs = 0;
    while (g_calls < calls) {
        Fake d;
        d.aql_on = !chance(20);
        long context = 0;
        const int engine_calls = 1 + (int)(rng() % 400);
        for (int c = 0; c < engine_calls && g_calls < calls; ++c, ++g_calls) {
            d.written_once = !chance(15);
            const int batch = 1 + (int)(rng() % 8);
            // mostly greedy or sampling plans, now and then any of the ten features
            unsigned mask = chance(50) ? 0u : (chance(60) ? (unsigned)(rng() % 8) : (unsigned)(rng() % 1024));
            const StepFeatures f = features_of(mask);
            const bool use_graph = !chance(10);
            std::vector<StepIn> steps(rng() % 9);
            for (StepIn &in : steps) {
                context += chance(30);
                AttnPlan sp;  // the plan moves with the context, as in a run
                sp.rq = batch <= 2 ? 1 : AD_RQ, sp.n_splits = 1 << (context / 40 % 4), sp.tokens_per_split = 64 * (int)(1 + context / 7 % 5);
                in.plan_key = sp.key();
                in.new_page = chance(20);
                in.refuse_reservation = chance(1), in.fail_capture = chance(2), in.refuse_program = chance(5), in.fail_submit = chance(1);
            }
            d.fail_next_drain = chance(1);
            const long before = d.decode_steps;
            const int rc = fake_decode(d, batch, f, use_graph, steps);
            ended[rc]++;
            if (rc == OK) require(d.decode_steps - before == (long)steps.size(), "a call that succeeded took every step");
            // every call ends with the queue idle, on success and on every failure but a failed drain (also one behind another failure)
            if (d.drain_failed) d.queue_busy = false;  // (the walk goes on from a drained engine; a real one is lost)
            require(!d.queue_busy, rc == OK ? "a call that succeeded ended with the queue busy"
                                   : rc == REFUSED ? "a call with a refused reservation ended with the queue busy" : "a call that failed ended with the queue busy");
            d.fail_next_drain = d.drain_failed = false;
            // captures equal cache misses (a miss whose capture failed took no step and left no plan)
            require(d.graph_captures == d.misses - d.lost_misses, "captures and cache misses differ");
            // what follows a call is stream-ordered: a read, a prefill, the next call's embedding gather
            d.stream_action("a stream launch behind a call while the queue is busy");
        }
        flushes += d.graph_cache_flushes, submitted += d.aql_steps, refused_programs += d.refused_programs;
        d.cache.clear();
        require(FakePlan::alive() == 0, "a cleared cache keeps plans alive");
    }
    require(flushes > 0 && submitted > 0 && refused_programs > 0, "the walk must reach a flush, the queue and a refused program");
    for (int rc = 0; rc < RC_COUNT; ++rc) require(ended[rc] > 0, "the walk must reach every way a call ends");
    std::printf("ok calls=%ld steps=%ld checks=%ld\n", g_calls, g_steps, g_checks);
    return 0;
}

// engine <aql_on> <written_once> <aql_why ...> | call <eager 0/1> <batch> <use_graph> <steps> <live feature mask> | step <n_splits> <tokens_per_split> <rq> <mask> <new_page>
static int run_trace() {
    Fake d;
    std::string aql_why;
    char line[1024];
    while (std::fgets(line, sizeof line, stdin)) {
        int a = 0, b = 0, used = 0;
        if (std::sscanf(line, "engine %d %d%n", &a, &b, &used) == 2) {
            d.cache.clear();
            d = Fake();
            d.aql_on = a != 0, d.written_once = b != 0;
            aql_why = line + used;
            while (!aql_why.empty() && (aql_why.back() == '\n' || aql_why.back() == ' ')) aql_why.pop_back();
            while (!aql_why.empty() && aql_why.front() == ' ') aql_why.erase(0, 1);
            continue;
        }
        int eager = 0, batch = 0, use_graph = 0, n = 0;
        unsigned live = 0;
        if (std::sscanf(line, "call %d %d %d %d %u", &eager, &batch, &use_graph, &n, &live) != 5) {
            std::printf("bad line: %s", line);
            return 1;
        }
        std::vector<StepIn> steps(n);
        unsigned mask = 0;
        for (StepIn &in : steps) {
            AttnPlan sp;
            int new_page = 0;
            if (!std::fgets(line, sizeof line, stdin) || std::sscanf(line, "step %d %d %d %u %d", &sp.n_splits, &sp.tokens_per_split, &sp.rq, &mask, &new_page) != 5) {
                std::printf("bad step: %s", line);
                return 1;
            }
            in.plan_key = sp.key(), in.new_page = new_page != 0;
        }
        const long before[5] = {d.decode_steps, d.graph_captures, d.graph_replays, d.aql_steps, d.graph_cache_flushes};
        // a profiled or checked step is a call of one eager step
        const int rc = fake_decode(d, batch, features_of(mask), !eager && use_graph, steps);
        ++g_calls;
        if (rc != OK || d.queue_busy) {  // (a recorded call succeeded)
            std::printf("call %ld failed\n", g_calls);
            return 1;
        }
        std::printf("%ld %ld %ld %ld %ld|%s\n", d.decode_steps - before[0], d.graph_captures - before[1], d.graph_replays - before[2], d.aql_steps - before[3],
                    d.graph_cache_flushes - before[4], replay_route_text(d.aql_on, aql_why, features_of(live)).c_str());
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "check")) return run_check(argc >= 3 ? (unsigned)std::atoi(argv[2]) : 1u, argc >= 4 ? std::atol(argv[3]) : 120000);
    if (argc >= 2 && !std::strcmp(argv[1], "trace")) return run_trace();
    std::printf("usage: replay_route_check check [seed [calls]] | trace < scenarios\n");
    return 2;
}
