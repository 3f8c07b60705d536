// The forest launch's plan (3d-beats_amd/csrc/rdf_launch_plan.hpp) worked out without a GPU: the invariants of plan_shape over a
// sweep of the smallest shapes at which each of its branches turns, the halo and LDS levels the source's comments quote, the
// sizes of a packed table, and select_kernel against a restatement of the rules and against the list of kernels.  Built and run
// by tests/test_launch_plan.py under the address + undefined-behaviour sanitizers, with no RDF_* variable in the environment
// (the knobs read it); exits non-zero on the first failed check.
#include "rdf_launch_plan.hpp"

#include <stdio.h>

#include <thread>
#include <vector>

struct Case {
    int Wl, Hl, r, n_img, T, D, C;
    bool packed, filtered, aligned;
    int block_knob, ps_deep_from, cus;
    uint32_t bad_last = 0, min_root = 0;
};

// what is under test, for a failing check's message: a line of text, or (g_what empty) the combination of the sweep
static thread_local char g_what[256] = "";
static thread_local const Case *g_case = nullptr;

[[noreturn]] static void fail(int line, const char *cond)
{
    fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, line, cond);
    if (g_what[0]) fprintf(stderr, "  at %s\n", g_what);
    else if (const Case *c = g_case)
        fprintf(stderr, "  at Wl %d Hl %d r %d n_img %d T %d D %d C %d packed %d filtered %d aligned %d block knob %d table's deep_from %d CUs %d\n",
                c->Wl, c->Hl, c->r, c->n_img, c->T, c->D, c->C, c->packed, c->filtered, c->aligned, c->block_knob, c->ps_deep_from, c->cus);
    _Exit(1);
}

#define CHECK(cond)                      \
    do {                                 \
        if (!(cond)) fail(__LINE__, #cond); \
    } while (0)

static const uint16_t *const kDepth = reinterpret_cast<const uint16_t *>(uintptr_t(0x100000));      // (never dereferenced)
static uint16_t *const kLabels = reinterpret_cast<uint16_t *>(uintptr_t(0x200000));
static const float *const kForest = reinterpret_cast<const float *>(uintptr_t(0x300000));
static const void *const kPacked = reinterpret_cast<const void *>(uintptr_t(0x40000000));           // 128-byte aligned
static const uint16_t *const kFilter = reinterpret_cast<const uint16_t *>(uintptr_t(0x500000));

static Request request_of(const Case &c)
{
    Request q = {};
    q.depth = c.aligned ? kDepth : kDepth + 1;
    q.n_img = c.n_img; q.dim_x = c.Wl * c.r; q.dim_y = c.Hl * c.r;
    q.packed = c.packed ? kPacked : nullptr;
    q.forest = c.packed ? nullptr : kForest;
    q.n_trees = c.T; q.max_depth = c.D; q.n_classes = c.C;
    q.filter = c.filtered ? kFilter : nullptr; q.filter_class = c.filtered ? 1 : -1;
    q.labels_out = kLabels; q.r = c.r; q.s = 1.0f;
    q.allow_tw = true;
    return q;
}

static PackedState table_of(const Case &c)
{
    PackedState ps;
    if (c.packed) {
        ps.deep_from = c.ps_deep_from; ps.exact_nodes = 0; ps.info_dev = kPacked; ps.generation = 7u;
        ps.deep_bad_last = c.bad_last; ps.deep_min_root = c.min_root;
    }
    return ps;
}

// Plans `c` the way plan_launch does (the argument checks first); false: the checks refuse it or there is nothing to do.
// (the block knob is the caller's to set: c.block_knob says what it is)
static bool plan_case(const Case &c, Plan *plan)
{
    g_case = &c;
    g_what[0] = 0;
    const Request q = request_of(c);
    CHECK(g_block_threads.value == c.block_knob);
    const int rc = check_common(q.depth, q.n_img, q.dim_x, q.dim_y, q.forest ? (const void *)q.forest : q.packed, q.n_trees, q.max_depth,
                                q.n_classes, q.labels_out, q.r);
    if (rc != 0) {
        CHECK(rc == RDF_ERR_TOO_LARGE && (long long)q.n_img * q.dim_x * q.dim_y >= (1ll << 31));       // (nothing else in the sweep is refused)
        return false;
    }
    *plan = Plan();
    CHECK(plan_shape(q, table_of(c), c.cus, nullptr, plan) == RDF_OK);
    return true;
}

// i / d == umulhi(i, magic) for every i < d * rows: looked at once per (d, rows)
static void check_magic(uint32_t d, uint32_t magic, uint32_t rows)
{
    static thread_local bool done[128][1024];
    CHECK(d < 128 && rows < 1024);
    if (done[d][rows]) return;
    done[d][rows] = true;
    for (uint32_t i = 0; i < d * rows; ++i) CHECK((uint32_t)(((unsigned long long)i * magic) >> 32) == i / d);
}

static void check_invariants(const Case &c, const Plan &p)
{
    const EvalArgs &a = p.a;
    const Geometry &g = p.g;
    // ---- tiling: the tiles cover the label map exactly once
    const int w_rem = c.Wl % 64;
    const bool folds = c.Wl > 64 && w_rem > 0 && w_rem <= 32;
    CHECK(a.fold == 0u || a.fold == 2u || a.fold == 4u);
    CHECK((a.fold != 0u) == folds);
    if (a.fold) {
        CHECK((int)a.tiles_x * 64 < c.Wl && c.Wl <= (int)a.tiles_x * 64 + 64 / (int)a.fold);     // the narrow tiles take the remainder, all of it
        CHECK((a.tiles_y_n - 1u) * g.tile_rows * a.fold < (uint32_t)c.Hl && (uint32_t)c.Hl <= a.tiles_y_n * g.tile_rows * a.fold);
    } else {
        CHECK(((int)a.tiles_x - 1) * 64 < c.Wl && c.Wl <= (int)a.tiles_x * 64);
        CHECK(a.tiles_y_n == 0u);
    }
    CHECK(g.tile_rows == (g.tw ? 8u / (uint32_t)c.T : (uint32_t)(g.block / 64 * a.rows_per_wave)));
    CHECK(a.rows_per_wave >= 1 && a.rows_per_wave <= kMaxRowsPerWave && (g.block == 256 || g.block == 512));
    CHECK((a.tiles_y - 1u) * g.tile_rows < (uint32_t)c.Hl && (uint32_t)c.Hl <= a.tiles_y * g.tile_rows);
    CHECK((unsigned long long)a.n_tiles == (unsigned long long)c.n_img * ((unsigned long long)a.tiles_x * a.tiles_y + a.tiles_y_n));
    // ---- LDS: [tile][node table][mailbox 32 B][pixel list | tree waves' exchange][slabs]
    const long long list_bytes = g.tw ? (long long)g.tile_rows * c.T * 256
                                      : p.compact_launch ? ((long long)g.block * a.rows_per_wave * 2 + g.tile_rows * 4 + 15) & ~15ll : 0;
    const long long slab_bytes = p.deep ? (long long)(g.block / 64) * 8192 : 0;
    const long long list_end = (long long)a.lds_list_off + list_bytes;
    CHECK(a.lds_nodes_off <= a.lds_mail_off && a.lds_mail_off <= a.lds_list_off && a.lds_mail_off + 32u == a.lds_list_off);
    CHECK(a.lds_slab_off % 1024u == 0u && (long long)a.lds_slab_off >= list_end);
    CHECK(a.lds_levels >= 0 && a.lds_levels <= c.D);
    CHECK((long long)a.lds_mail_off - a.lds_nodes_off == (a.lds_levels > 0 ? (long long)c.T * (1ll << a.lds_levels) * 16 : 0));
    // the budget of the workgroup size, with no knob set: three 512-thread or five 256-thread workgroups per CU; beside the slabs
    // two or four
    const long long budget = p.deep ? (g.block == 512 ? 81920 - 65536 - 1024 : 40960 - 32768 - 1024) : (g.block == 512 && !g.tw ? 54600 : 32700);
    CHECK(p.lds_bytes == (p.deep ? (long long)a.lds_slab_off + slab_bytes : list_end));
    CHECK(list_end <= budget);
    CHECK(p.lds_bytes <= 160 * 1024);
    // ---- the staged tile, in front of the node table
    if (a.tw > 0) {
        CHECK((long long)a.th * a.twp * 2 <= (long long)a.lds_nodes_off);
        CHECK(a.tw >= 63 * c.r + 1 + 2 * a.halo && a.twp >= a.tw);
        CHECK(a.th == ((int)g.tile_rows - 1) * c.r + 1 + 2 * a.halo);
        if (a.fold) {
            CHECK((long long)a.th_n * a.twp_n * 2 <= (long long)a.lds_nodes_off);
            CHECK(a.halo_xn >= 0 && a.halo_xn <= a.halo);
            CHECK(a.tw_n >= (64 / (int)a.fold - 1) * c.r + 1 + 2 * a.halo_xn && a.twp_n >= a.tw_n);
            CHECK(a.th_n == ((int)(g.tile_rows * a.fold) - 1) * c.r + 1 + 2 * a.halo);
        }
    } else {
        CHECK(a.lds_nodes_off == 0u && a.stage_tw8 == 0u);
    }
    // ---- 16-byte staging
    if (a.stage_tw8 > 0u) {
        CHECK(c.aligned && (c.Wl * c.r) % 8 == 0 && a.halo % 8 == 0);
        CHECK(a.stage_tw8 * 8u == (uint32_t)a.tw && (a.twp * 2) % 16 == 0);
        check_magic(a.stage_tw8, a.stage_magic, (uint32_t)a.th);
        if (a.fold) {
            CHECK(a.stage_tw8_n * 8u == (uint32_t)a.tw_n && (a.twp_n * 2) % 16 == 0);
            check_magic(a.stage_tw8_n, a.stage_magic_n, (uint32_t)a.th_n);
        }
    }
    // ---- deep blocks
    const int cpad = (c.C + 3) & ~3;
    if (p.deep) {
        const int R0 = c.D - (cpad == 4 ? 2 : 1);
        CHECK(c.packed && !g.tw && c.bad_last == 0u && deep_possible(c.T, c.D, cpad));
        CHECK(a.deep != nullptr && a.deep_from <= R0 && a.deep_from >= 0 && (R0 - a.deep_from) % 3 == 0);
        CHECK(a.lds_levels <= a.deep_from);
        CHECK((int)c.min_root <= a.deep_from);
    } else {
        CHECK(a.deep == nullptr);
    }
}

static std::atomic<int> g_planned{0}, g_refused{0}, g_deep{0}, g_tw{0};

// every combination of one label width under one setting of the block knob
static void sweep_width(int Wl, int knob)
{
    const int Hls[] = {1, 7, 16, 33, 480}, rs[] = {1, 2, 3}, n_imgs[] = {1, 8, 64, 2048}, Ts[] = {1, 2, 3, 4, 6, 8};
    const int Ds[] = {1, 4, 5, 20, 24, 25, 27}, Cs[] = {1, 4, 5, 8, 9, 16}, deep_froms[] = {-1, 0, 9}, cuss[] = {8, 256};
    Case c = {};
    Plan p;
    int planned = 0, refused = 0, deep = 0, tw = 0;
    for (int Hl : Hls) for (int r : rs) for (int n_img : n_imgs) for (int T : Ts) for (int D : Ds) for (int C : Cs)
    for (int packed = 0; packed < 2; ++packed) for (int filtered = 0; filtered < 2; ++filtered)
    for (int deep_from : deep_froms) for (int cus : cuss) for (int aligned = 0; aligned < 2; ++aligned) {
        if (!packed && deep_from != -1) continue;       // (only a packed table has a choice: the same plan three times)
        c.Wl = Wl; c.Hl = Hl; c.r = r; c.n_img = n_img; c.T = T; c.D = D; c.C = C;
        c.packed = packed; c.filtered = filtered; c.aligned = aligned; c.block_knob = knob; c.ps_deep_from = deep_from; c.cus = cus;
        if (!plan_case(c, &p)) { ++refused; continue; }
        check_invariants(c, p);
        ++planned; deep += p.deep; tw += p.g.tw;
    }
    g_planned += planned; g_refused += refused; g_deep += deep; g_tw += tw;
}

static void sweep_invariants()
{
    // (the knob is process-wide, so its three settings go one after the other; the widths of one setting share the cores)
    for (int knob : {0, 256, 512}) {
        g_block_threads.value = knob;
        std::vector<std::thread> threads;
        for (int Wl : {1, 63, 64, 65, 80, 96, 97, 100, 128, 848}) threads.emplace_back(sweep_width, Wl, knob);
        for (std::thread &t : threads) t.join();
    }
    g_block_threads.value = 0;
    CHECK(g_deep > 0 && g_tw > 0 && g_refused > 0);
    // a table whose blocks cannot serve the forest is never planned deep: a level D-1 node that is not a plain two-leaf node, or
    // exact nodes below the last block's root; exact nodes higher up move the start down to their level
    Plan p;
    Case c = {848, 480, 1, 64, 4, 20, 4, true, false, true, 0, 9, 256};
    CHECK(plan_case(c, &p) && p.deep && p.a.deep_from == 9);
    c.bad_last = 1u;
    CHECK(plan_case(c, &p) && !p.deep);
    c.bad_last = 0u; c.min_root = 19u;      // R0 = 18
    CHECK(plan_case(c, &p) && !p.deep);
    c.min_root = 13u;
    CHECK(plan_case(c, &p) && p.deep && p.a.deep_from == 15);
    check_invariants(c, p);
}

// The arithmetic behind rdf_forest_packed_bytes, restated: two tables per heap slot (16-byte hot record, PDF rows of the classes
// padded to four); up to four classes: the 64-byte records of the deepest level and a 64-byte trailer; up to eight classes and
// 5 to 24 levels: the deep blocks on a 128-byte boundary, a zero line and a 128-byte trailer; last the 128-byte info block.
static void check_sizes()
{
    for (int T = 1; T <= 8; ++T) for (int D = 1; D <= 27; ++D) for (int C = 1; C <= 16; ++C) {
        snprintf(g_what, sizeof(g_what), "T %d D %d C %d", T, D, C);
        const size_t cpad = (size_t)((C + 3) / 4 * 4);
        size_t n = ((size_t)T << D) * (16 + 2 * cpad * 4);
        if (cpad == 4 && D >= 2) n += ((size_t)T << (D - 1)) * 64 + 64;
        n = (n + 127) / 128 * 128;
        CHECK(deep_offset(T, D, C) == n && deep_offset(T, D, C) % 128 == 0);
        if (cpad <= 8 && D >= 5 && D <= 24) {
            const int R0 = D - (cpad == 4 ? 2 : 1);
            size_t lines = (size_t)T << R0;                         // the last blocks,
            for (int R = R0 - 3; R >= 0; R -= 3) lines += (size_t)T << R;   // the three-level blocks above them, root level by root level
            CHECK(deep_total_lines(T, D, (int)cpad) == lines);
            n += (lines + 2) * 128;
        } else {
            CHECK(deep_bytes(T, D, C) == 0);
        }
        CHECK(info_offset(T, D, C) == n);
        CHECK(info_offset(T, D, C) + sizeof(PackInfo) == n + 128);
    }
}

// The halo and LDS levels the comments of choose_geometry and lay_out_lds quote, for the frames of the metric (848 x 480) in a
// batch that fills the chip.  Each expected pair is worked out by hand from the formulas ("Forest launch:
// the plan in a host-only header", has the derivations and the three places where the comment's number is not the plan's).
static void check_quoted_numbers()
{
    struct Quoted { const char *what; int T, r, knob, deep_from, halo, levels; };
    const Quoted quoted[] = {
        {"256 threads: four trees 7 levels + 32 px", 4, 1, 256, -1, 32, 7},
        {"512 threads: 56 px with 7 levels", 4, 1, 0, -1, 56, 7},
        {"256 threads: eight trees 5 levels + 40 px", 8, 1, 256, -1, 40, 5},
        {"512 threads, eight trees: 56 px; the comment says 5 levels, the budget holds 6", 8, 1, 0, -1, 56, 6},
        {"labels_reduce 2, 512 threads: 32 px; the comment's 6 levels were a forced setting, the budget holds 8", 4, 2, 0, -1, 32, 8},
        {"deep blocks, 512 threads, eight trees: 24 px, 4 levels", 8, 1, 0, 9, 24, 4},
        {"deep blocks, 512 threads: 16 px, 6 levels (at least the 5 the comment names)", 4, 1, 0, 9, 16, 6},
        {"deep blocks, 256 threads: the comment's 8 px miss the tile's budget by 32 bytes, the plan takes 6 px; 5 levels", 4, 1, 256, 9, 6, 5},
    };
    for (const Quoted &e : quoted) {
        const Case c = {848 / e.r, 480 / e.r, e.r, 64, e.T, 20, 4, true, false, true, e.knob, e.deep_from, 256};
        Plan p;
        g_block_threads.value = e.knob;
        CHECK(plan_case(c, &p));
        snprintf(g_what, sizeof(g_what), "%s: the plan has %d px, %d levels", e.what, p.a.halo, p.a.lds_levels);
        CHECK(p.g.big && p.g.block == (e.knob ? e.knob : 512) && p.deep == (e.deep_from > 0));
        CHECK(p.a.halo == e.halo);
        CHECK(p.a.lds_levels == e.levels);
    }
    g_block_threads.value = 0;
}

// ---- selection
static bool listed(const KernelKey &k) { return kernel_index(k) >= 0; }

static void check_selection()
{
    CHECK(kNumForestKernels == 65 && kNumForestKernels < 75);
    for (int i = 0; i < kNumForestKernels; ++i)
        for (int j = i + 1; j < kNumForestKernels; ++j) CHECK(!(kForestKernels[i] == kForestKernels[j]));
    bool taken[kNumForestKernels] = {};
    // trees in a lane by the width wanted (1..4; more: 4), as the launch functions chose them: packed forests of up to eight
    // classes have a kernel of every width, sixteen classes and the reference layout one and four, deep blocks two to four
    enum { kPacked8, kPacked16, kReference, kDeep };
    static const int lane_trees[4][5] = {{0, 1, 2, 3, 4}, {0, 1, 4, 4, 4}, {0, 1, 4, 4, 4}, {0, 2, 2, 3, 4}};
    Plan p;
    for (int packed = 0; packed < 2; ++packed) for (int C = 1; C <= 16; ++C) for (int T = 1; T <= 8; ++T)
    for (int compact = 0; compact < 2; ++compact) for (int deep = 0; deep < 2; ++deep) for (int stats = 0; stats < 2; ++stats)
    for (int block = 256; block <= 512; block += 256) for (int tw = 0; tw < 2; ++tw) for (int knob = 0; knob <= 4; ++knob) {
        // what a plan can be: a pixel list, deep blocks and tree waves need a packed table; deep blocks at most eight classes; counters
        // no pixel list; tree waves 512 threads, two to four trees, up to eight classes and nothing else; reference-layout counters 256 threads
        if (!packed && (compact || deep || tw)) continue;
        if (deep && C > 8) continue;
        if (stats && compact) continue;
        if (tw && (block != 512 || T < 2 || T > 4 || C > 8 || compact || deep || stats)) continue;
        if (stats && !packed && block != 256) continue;
        snprintf(g_what, sizeof(g_what), "packed %d C %d T %d pixel list %d deep %d counters %d block %d tree waves %d group knob %d",
                 packed, C, T, compact, deep, stats, block, tw, knob);
        p = Plan();
        p.packed = packed; p.compact_launch = compact; p.deep = deep; p.stats = stats;
        p.g.block = block; p.g.tw = tw;
        p.a.C = C; p.a.T = T; p.a.cpad = (C + 3) & ~3;
        g_group.value = knob;
        const KernelKey got = select_kernel(p);
        if (stats && packed && C > 4) {     // no such kernel: RDF_ERR_BAD_ARG
            CHECK(got.block == 0);
            continue;
        }
        const int width = knob > 0 ? knob : T == 1 ? 1 : T == 2 ? 2 : (T == 3 || T == 6) ? 3 : 4;
        const int cmax_packed = C <= 4 ? 4 : C <= 8 ? 8 : 16;
        KernelKey want;
        if (tw) want = {512, true, cmax_packed, false, 1, false, 1, true, false};
        else if (stats) want = {block, packed != 0, 4, true, 4, false, 1, false, deep != 0};
        else if (!packed) want = {block, false, C <= 4 ? 4 : 16, false, lane_trees[kReference][width], false, 1, false, false};
        else if (compact) want = {block, true, cmax_packed, false, 4, true, 1, false, deep != 0};
        else want = {block, true, cmax_packed, false, lane_trees[deep ? kDeep : cmax_packed == 16 ? kPacked16 : kPacked8][width], false, 1, false, deep != 0};
        CHECK(got == want);
        CHECK(listed(got));
        taken[kernel_index(got)] = true;
    }
    g_group.value = 0;
    for (int nl = 2; nl <= 3; ++nl) for (int cmax = 4; cmax <= 8; cmax += 4) for (int tw_all = 0; tw_all < 2; ++tw_all) {
        snprintf(g_what, sizeof(g_what), "%d layers, %d classes, tree waves %d", nl, cmax, tw_all);
        const KernelKey got = select_layers_kernel(nl, cmax, tw_all);
        const KernelKey want = {tw_all ? 512 : 256, true, cmax, false, tw_all ? 1 : 4, false, nl, tw_all != 0, false};
        CHECK(got == want && listed(got));
        taken[kernel_index(got)] = true;
    }
    for (int i = 0; i < kNumForestKernels; ++i) {
        snprintf(g_what, sizeof(g_what), "kForestKernels[%d]: no launch takes it", i);
        CHECK(taken[i]);
    }
}

int main()
{
    check_sizes();
    check_quoted_numbers();
    check_selection();
    sweep_invariants();
    printf("launch plan ok: %d plans (%d deep, %d tree waves), %d requests refused as too large\n", g_planned.load(), g_deep.load(), g_tw.load(),
           g_refused.load());
    return 0;
}
