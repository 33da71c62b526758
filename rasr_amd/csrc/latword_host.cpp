// latword_host.cpp -- lattice word measures, host side: the checks and the plan of a call (no device).
//
// The discover order is latpost_plan's (latpost_host.cpp restates DfsState::dfs); it is called with weights of zero and no final state,
// which its walk does not read.  What this plan adds:
//   records    per segment the reached arcs with start < end in discover order (states in discover order, within a state arc order), sorted
//              stably by label: a label's records stand in the order in which TimeframeErrorDfsState::discoverState feeds its collectors
//              (Lattice/TimeframeError.cc:124-142).  Host memory holds the labels and the times, so the sort is std::stable_sort here.
//   rows       a (segment, label) owns the cells of the frames its records span; the rows of a segment ascend by label.
//   units      a row's blocks of 64 frames, one wave each; for a row of kLwListArcs records and more the number of records that touch each
//              block, so that the device's ballot pass has a place to write their list.
//   intervals  approximate word accuracy: the distinct (start, end, label) of the correct lattice's arcs, sorted, with a running maximum
//              of the ends (ApproximateWordAccuracyAutomaton::LatticeToActiveStates, Lattice/Accuracy.cc:430-441).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"
#include "latpost_plan.hpp"
#include "latword_plan.hpp"

namespace amx {

namespace {

// the checks of one set of lattices and its walk
int lw_walk(const amx_latword_lattices* t, const char* who, const char* what, LatPlan* lp) {
    AMX_REQUIRE(t, AMX_ERR_INVALID, "%s: NULL %s lattices", who, what);
    AMX_REQUIRE(t->n_seg >= 0, AMX_ERR_INVALID, "%s: %s: n_seg %d", who, what, t->n_seg);
    AMX_REQUIRE(t->state_offsets && t->arc_offsets, AMX_ERR_INVALID, "%s: %s: NULL state_offsets or arc_offsets", who, what);
    AMX_REQUIRE(t->state_offsets[0] == 0, AMX_ERR_INVALID, "%s: %s: state_offsets[0] must be 0", who, what);
    for (int g = 0; g < t->n_seg; ++g)
        AMX_REQUIRE(t->state_offsets[g + 1] >= t->state_offsets[g], AMX_ERR_INVALID, "%s: %s: state_offsets descend at segment %d", who, what, g);
    const long n_states = t->state_offsets[t->n_seg];
    for (long i = 0; i < n_states; ++i)
        AMX_REQUIRE(t->arc_offsets[i + 1] >= t->arc_offsets[i], AMX_ERR_INVALID, "%s: %s: arc_offsets descend at state %ld", who, what, i);
    const long n_arcs = t->arc_offsets[n_states];
    AMX_REQUIRE(n_states == 0 || t->state_time, AMX_ERR_INVALID, "%s: %s: NULL state_time", who, what);
    AMX_REQUIRE(n_arcs == 0 || t->arc_label, AMX_ERR_INVALID, "%s: %s: NULL arc_label", who, what);
    const std::vector<float>   weight((size_t)n_arcs + 1, 0.f);
    const std::vector<uint8_t> final_flag((size_t)n_states + 1, 0);
    AMX_TRY(latpost_plan(AMX_LATPOST_LOG, t->n_seg, t->state_offsets, t->arc_offsets, t->arc_target, weight.data(), nullptr, t->initial, final_flag.data(),
                         nullptr, nullptr, who, lp));
    for (int g = 0; g < t->n_seg; ++g) {
        const long s0 = t->state_offsets[g];
        for (long s = s0; s < t->state_offsets[g + 1]; ++s) {
            AMX_REQUIRE(t->state_time[s] >= 0 && t->state_time[s] < (1 << 30), AMX_ERR_INVALID, "%s: %s: segment %d: time %d of state %ld is outside [0, 2^30)", who,
                        what, g, t->state_time[s], s - s0);
            for (long a = t->arc_offsets[s]; a < t->arc_offsets[s + 1]; ++a)
                AMX_REQUIRE(t->state_time[s0 + t->arc_target[a]] >= t->state_time[s], AMX_ERR_INVALID,
                            "%s: %s: segment %d: state_time decreases along arc %ld of state %ld (%d after %d)", who, what, g, a - t->arc_offsets[s], s - s0,
                            t->state_time[s0 + t->arc_target[a]], t->state_time[s]);
        }
    }
    return AMX_OK;
}

// a segment's states in discover order
void lw_discover(const LatPlan& lp, long s0, int n, int g, std::vector<int32_t>* discover) {
    discover->assign((size_t)lp.info[(size_t)g].states_reached, -1);
    for (int s = 0; s < n; ++s)
        if (lp.discover_index[(size_t)(s0 + s)] >= 0)
            (*discover)[(size_t)lp.discover_index[(size_t)(s0 + s)]] = s;
}

int lw_table(const amx_latword_lattices& t, const LatPlan& lp, const char* who, LwTable* out) {
    std::vector<int32_t>                       discover;
    std::vector<std::pair<int32_t, LwRec>>     fed;
    out->seg_row.assign((size_t)t.n_seg + 1, 0);
    for (int g = 0; g < t.n_seg; ++g) {
        const long s0 = t.state_offsets[g];
        lw_discover(lp, s0, (int)(t.state_offsets[g + 1] - s0), g, &discover);
        fed.clear();
        for (int u : discover)
            for (long a = t.arc_offsets[s0 + u]; a < t.arc_offsets[s0 + u + 1]; ++a) {
                const int s = t.state_time[s0 + u], e = t.state_time[s0 + t.arc_target[a]];
                if (s < e)
                    fed.push_back({t.arc_label[a], LwRec{s, e, (int)a}});
            }
        std::stable_sort(fed.begin(), fed.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        for (size_t i = 0; i < fed.size(); ++i) {
            if (i == 0 || fed[i].first != fed[i - 1].first)
                out->row.push_back(LwRow{(int)out->rec.size(), 0, INT_MAX, 0, g, fed[i].first, 0});
            LwRow& r = out->row.back();
            ++r.n_rec;
            r.lo = std::min(r.lo, fed[i].second.start), r.hi = std::max(r.hi, fed[i].second.end);
            out->rec.push_back(fed[i].second);
        }
        out->seg_row[(size_t)g + 1] = (int)out->row.size();
    }
    std::vector<int> count;
    for (size_t ri = 0; ri < out->row.size(); ++ri) {
        LwRow& r  = out->row[ri];
        r.cell0   = out->n_cells;
        out->n_cells += r.hi - r.lo + 1;
        const int    n_blocks = (r.hi - r.lo + kLwBlockFrames - 1) / kLwBlockFrames;
        const bool   wide     = r.n_rec >= kLwListArcs;
        const size_t first    = out->unit.size();
        if (wide) {
            count.assign((size_t)n_blocks, 0);
            for (int i = r.rec0; i < r.rec0 + r.n_rec; ++i)
                for (int b = (out->rec[(size_t)i].start - r.lo) / kLwBlockFrames; b <= (out->rec[(size_t)i].end - 1 - r.lo) / kLwBlockFrames; ++b)
                    ++count[(size_t)b];
        }
        for (int b = 0; b < n_blocks; ++b) {
            out->unit.push_back(LwUnit{(int)ri, r.lo + b * kLwBlockFrames, (int)out->n_list, wide ? count[(size_t)b] : -1});
            if (wide) {
                out->wide_unit.push_back((int)(first + (size_t)b));
                out->n_list += count[(size_t)b];
            }
        }
    }
    AMX_REQUIRE(out->n_cells < (1ll << 30) && out->n_list < (1ll << 30) && out->unit.size() < ((size_t)1 << 30), AMX_ERR_UNSUPPORTED,
                "%s: a table of %lld cells in %zu blocks is more than one call takes", who, out->n_cells, out->unit.size());
    return AMX_OK;
}

}  // namespace

int latword_plan(const amx_latword_cfg& cfg, const amx_latword_lattices* lat, const amx_latword_lattices* correct, const int32_t* short_pause_label,
                 int n_short_pause, const char* who, LwPlan* out) {
    const bool timeframe = cfg.mode == AMX_LATWORD_TIMEFRAME_ERROR_SUM || cfg.mode == AMX_LATWORD_TIMEFRAME_ERROR_MAX;
    const bool approximate = cfg.mode == AMX_LATWORD_APPROXIMATE_WORD;
    LwPlan&    p = *out;
    p            = LwPlan();
    LatPlan lp, lp_ref;
    AMX_TRY(lw_walk(lat, who, "the", &lp));
    if (!timeframe) {
        AMX_REQUIRE(correct, AMX_ERR_INVALID, "%s: the accuracy modes need the correct lattices", who);
        AMX_TRY(lw_walk(correct, who, "the correct", &lp_ref));
        AMX_REQUIRE(correct->n_seg == lat->n_seg, AMX_ERR_INVALID, "%s: %d correct lattices for %d lattices", who, correct->n_seg, lat->n_seg);
    }
    AMX_REQUIRE(n_short_pause >= 0 && (n_short_pause == 0 || short_pause_label), AMX_ERR_INVALID, "%s: %d short pause labels, or a NULL list", who, n_short_pause);
    const amx_latword_lattices& t = *lat;
    p.n_seg = t.n_seg, p.n_states = lp.n_states, p.n_arcs = lp.n_arcs;
    p.info.assign((size_t)t.n_seg, amx_latword_info{});
    p.arc_start.assign((size_t)p.n_arcs, 0), p.arc_end.assign((size_t)p.n_arcs, 0), p.arc_row.assign((size_t)p.n_arcs, kLwArcUnreached);
    p.arc_seg.assign((size_t)p.n_arcs, 0);
    p.seg_interval.assign((size_t)t.n_seg + 1, 0);
    if (timeframe)
        AMX_TRY(lw_table(t, lp, who, &p.hyp));
    else if (!approximate)
        AMX_TRY(lw_table(*correct, lp_ref, who, &p.ref));
    const LwTable&       table = timeframe ? p.hyp : p.ref;
    std::vector<int32_t> pauses(short_pause_label, short_pause_label + (approximate ? n_short_pause : 0)), discover;
    std::sort(pauses.begin(), pauses.end());
    for (int g = 0; g < t.n_seg; ++g) {
        const long        s0   = t.state_offsets[g];
        const int         n    = (int)(t.state_offsets[g + 1] - s0);
        amx_latword_info& info = p.info[(size_t)g];
        info.states_reached    = lp.info[(size_t)g].states_reached;
        info.states_unreached  = n - info.states_reached;
        info.arcs_reached      = lp.info[(size_t)g].arcs_reached;
        const LwRow *r0 = table.row.data() + (table.seg_row.empty() ? 0 : table.seg_row[(size_t)g]),
                    *r1 = table.row.data() + (table.seg_row.empty() ? 0 : table.seg_row[(size_t)g + 1]);
        info.labels = (int)(r1 - r0);
        for (const LwRow* r = r0; r < r1; ++r)
            for (int i = r->rec0; i < r->rec0 + r->n_rec; ++i)
                info.feeds += table.rec[(size_t)i].end - table.rec[(size_t)i].start;
        if (approximate) {
            // the correct lattice's distinct intervals
            const amx_latword_lattices& c  = *correct;
            const long                  c0 = c.state_offsets[g];
            const size_t                at = p.interval.size();
            for (long s = c0; s < c.state_offsets[g + 1]; ++s)
                if (lp_ref.discover_index[(size_t)s] >= 0)
                    for (long a = c.arc_offsets[s]; a < c.arc_offsets[s + 1]; ++a)
                        if (c.state_time[s] < c.state_time[c0 + c.arc_target[a]])
                            p.interval.push_back(LwInterval{c.state_time[s], c.state_time[c0 + c.arc_target[a]], c.arc_label[a], 0});
            auto less = [](const LwInterval& x, const LwInterval& y) {
                return x.start != y.start ? x.start < y.start : x.end != y.end ? x.end < y.end : x.label < y.label;
            };
            std::sort(p.interval.begin() + (long)at, p.interval.end(), less);
            p.interval.erase(std::unique(p.interval.begin() + (long)at, p.interval.end(), [&](const LwInterval& x, const LwInterval& y) { return !less(x, y) && !less(y, x); }),
                             p.interval.end());
            int maxend = 0;
            for (size_t i = at; i < p.interval.size(); ++i)
                p.interval[i].maxend = maxend = std::max(maxend, p.interval[i].end);
            info.intervals = (int)(p.interval.size() - at);
        }
        p.seg_interval[(size_t)g + 1] = (int)p.interval.size();
        for (int s = 0; s < n; ++s) {
            const bool reached = lp.discover_index[(size_t)(s0 + s)] >= 0;
            for (long a = t.arc_offsets[s0 + s]; a < t.arc_offsets[s0 + s + 1]; ++a) {
                const int b = t.state_time[s0 + s], e = t.state_time[s0 + t.arc_target[a]];
                p.arc_start[(size_t)a] = b, p.arc_end[(size_t)a] = e, p.arc_seg[(size_t)a] = g;
                if (reached && e > info.frames)
                    info.frames = e;
                if (!reached)
                    continue;
                if (approximate)
                    p.arc_row[(size_t)a] = b < e && !std::binary_search(pauses.begin(), pauses.end(), t.arc_label[a]) ? 0 : kLwArcUnreached;
                else {
                    const LwRow* r = std::lower_bound(r0, r1, t.arc_label[a], [](const LwRow& x, int32_t l) { return x.label < l; });
                    p.arc_row[(size_t)a] = b < e && r < r1 && r->label == t.arc_label[a] ? (int)(r - table.row.data()) : kLwArcNoRow;
                }
                if (timeframe && e - b >= kLwWaveFrames)
                    p.long_arc.push_back((int32_t)a);
            }
        }
    }
    return AMX_OK;
}

}  // namespace amx

extern "C" {

void amx_latword_cfg_default(amx_latword_cfg* cfg) {
    if (!cfg)
        return;
    cfg->mode          = AMX_LATWORD_TIMEFRAME_ERROR_SUM;
    cfg->normalization = 0.f;
}

void amx_latword_kernel_shape(int* block_frames, int* list_arcs, int* wave_arc_frames) {
    if (block_frames)
        *block_frames = amx::kLwBlockFrames;
    if (list_arcs)
        *list_arcs = amx::kLwListArcs;
    if (wave_arc_frames)
        *wave_arc_frames = amx::kLwWaveFrames;
}

}  // extern "C"
