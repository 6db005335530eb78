// spectrum_plan.h — the rows and batches of one mdhip_velocity_spectrum call (velocity_spectrum.hip), decided from the group
// table alone.
//
// Every entity of a group has three time series, one per axis. The series are the ROWS of a time-major copy of the
// trajectory, ordered (axis, group, entity ascending): row = axis * n_rows + group_row0[group] + (the entity's rank inside
// its group), so that every (axis, group) is ONE contiguous range of rows although the groups themselves are interleaved
// in the trajectory (atom types inside molecules). Entities of group -1 have no row.
// The time-major copy is made in BATCHES of whole rows whose series and transform buffers stay within a byte bound. A
// batch is one axis of a CUT: a range of consecutive entities [e_lo, e_hi) with all their groups, so that the pass that
// fills it reads every line of the trajectory once, whatever the interleaving. (A batch of ONE group would fetch a line
// that holds three atom types for a third of its doubles, and the other two batches would fetch it again: 1.22 against
// 0.50 ms per batch at 50 000 entities x 10 000 frames.) Inside the batch buffer the rows keep the order (group,
// entity): buffer row = ent_row[e] + shift[group], and the rows of group g are the contiguous range [seg[g], seg[g + 1])
// — what the column sums of |X_k|^2 over a group take. The cuts are the same for the three axes; the batches run axis
// after axis, cut after cut, and cover the 3 * n_rows rows once.
// Everything here is host arithmetic on plain values (no HIP header, no context), in the form of shape_plan.h:
// tests/native/spectrum_plan_main.cpp includes this header with g++ and walks it under sanitizers. An unnamed namespace, as
// the kernels that take SpGroups and SpShift: their symbols keep their names.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

constexpr int SP_MAX_GROUPS = 16;
constexpr long long SP_MAX_BATCH_ROWS = 1ll << 30;  // rows of a batch at most (the transforms count them in an int)

// GROUPS: n_groups outside 1 .. SP_MAX_GROUPS; ENTITY: entity `bad_entity` names a group outside -1 .. n_groups - 1 (the
// FIRST such entity); LENGTH: L is no power of two within [4, 2^30), or below n_frames + max_lag, or max_lag outside
// 0 .. n_frames - 1, or n_frames < 1, or n_ent < 0
enum SpPlanError { SP_PLAN_OK = 0, SP_PLAN_GROUPS, SP_PLAN_ENTITY, SP_PLAN_LENGTH };

// first row of every group inside an axis (row0[n_groups .. SP_MAX_GROUPS] = n_rows): passed to kernels by value
struct SpGroups {
    long long row0[SP_MAX_GROUPS + 1];
};

// buffer row of an entity of group g inside a cut = ent_row[e] + add[g]: passed to kernels by value
struct SpShift {
    long long add[SP_MAX_GROUPS];
};

struct SpCut {
    long long e_lo, e_hi;              // the entities of the cut (the first and the last one are grouped)
    long long rows;                    // grouped entities among them = rows of a batch of this cut
    long long seg[SP_MAX_GROUPS + 1];  // first buffer row of every group (seg[n_groups ..] = rows)
    SpShift shift;
};

struct SpPlan {
    std::vector<long long> ent_row;  // [n_ent]: the entity's row inside an axis, -1 for an entity of no group
    SpGroups groups;
    long long n_rows = 0;            // grouped entities = rows per axis
    long long row_bytes = 0;         // device bytes of one row: its series and its share of the transform buffers
    long long max_rows = 0;          // rows of the largest batch
    std::vector<SpCut> cuts;         // batch b = (axis b / cuts.size(), cut b % cuts.size())
    int error = SP_PLAN_OK;
    long long bad_entity = -1;
    long long rows_total() const { return 3 * n_rows; }
    long long n_batches() const { return 3 * (long long)cuts.size(); }
};

inline bool sp_lengths_ok(int64_t n_frames, int64_t n_ent, int64_t L, int64_t max_lag)
{
    return n_frames >= 1 && n_ent >= 0 && L >= 4 && L < (1ll << 30) && (L & (L - 1)) == 0 && max_lag >= 0 &&
           max_lag <= n_frames - 1 && L >= n_frames + max_lag;
}

// transform_buffers: buffers of L / 2 complex points a series needs (1: the two-pass form, 2: the packed transform);
// batch_bytes: the bound of a batch (a batch of ONE row may exceed it: a series is never cut)
inline SpPlan spectrum_plan(int64_t n_frames, int64_t n_ent, int n_groups, const int32_t *ent_group, int64_t L, int64_t max_lag,
                            int transform_buffers, long long batch_bytes)
{
    SpPlan pl;
    for (long long &r : pl.groups.row0) r = 0;
    if (n_groups < 1 || n_groups > SP_MAX_GROUPS) {
        pl.error = SP_PLAN_GROUPS;
        return pl;
    }
    if (!sp_lengths_ok(n_frames, n_ent, L, max_lag)) {
        pl.error = SP_PLAN_LENGTH;
        return pl;
    }
    long long count[SP_MAX_GROUPS] = {0};
    for (int64_t e = 0; e < n_ent; ++e) {
        const int32_t g = ent_group[e];
        if (g < -1 || g >= n_groups) {
            pl.error = SP_PLAN_ENTITY, pl.bad_entity = e;
            return pl;
        }
        if (g >= 0) ++count[g];
    }
    long long next[SP_MAX_GROUPS] = {0};
    for (int g = 0; g <= SP_MAX_GROUPS; ++g) {
        pl.groups.row0[g] = pl.n_rows;
        if (g < n_groups) next[g] = pl.n_rows, pl.n_rows += count[g];
    }
    pl.row_bytes = ((long long)n_frames + (long long)transform_buffers * L) * 8;
    const long long per = std::max<long long>(1, std::min<long long>(SP_MAX_BATCH_ROWS, batch_bytes / pl.row_bytes));
    pl.ent_row.resize((size_t)n_ent);
    // the cuts: `per` grouped entities each, the last one what is left; first[g]: the row of the cut's first entity of g
    long long in_cut[SP_MAX_GROUPS] = {0}, first[SP_MAX_GROUPS] = {0};
    SpCut cut{};
    long long last_grouped = -1;
    auto close = [&](long long e_hi) {
        cut.e_hi = e_hi;
        long long at = 0;
        for (int g = 0; g <= SP_MAX_GROUPS; ++g) {
            cut.seg[g] = at;
            if (g < n_groups) {
                cut.shift.add[g] = at - first[g];
                at += in_cut[g], in_cut[g] = 0;
            } else if (g < SP_MAX_GROUPS) {
                cut.shift.add[g] = 0;
            }
        }
        pl.max_rows = std::max(pl.max_rows, cut.rows);
        pl.cuts.push_back(cut);
        cut = SpCut{};
    };
    for (int64_t e = 0; e < n_ent; ++e) {
        const int32_t g = ent_group[e];
        if (g < 0) {
            pl.ent_row[(size_t)e] = -1;
            continue;
        }
        const long long row = next[g]++;
        pl.ent_row[(size_t)e] = row;
        if (cut.rows == 0) cut.e_lo = e;
        if (in_cut[g]++ == 0) first[g] = row;
        last_grouped = e;
        if (++cut.rows == per) close(e + 1);
    }
    if (cut.rows > 0) close(last_grouped + 1);  // (the last entity of a cut is grouped: entities of no group behind it are never read)
    return pl;
}

}  // namespace
