// GPU-less check of the first-writer geometry of the owner-computes push (csrc/owner_geom.hpp: fresh_range, bricks_over), by brute
// force: build the ownership map of the lattice from the boxes of the interior bricks and the order of the colour launches, and
// compare it with what the functions say.  Stand-alone: tests/test_first_writer_geom.py builds it with -fsanitize=address,undefined
// and runs it.  Exit status 0 and a line "ok ..." when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "owner_geom.hpp"

using namespace ip::owner;

static long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static int origin(const BrickGrid &g, int d, int bk) { return brick_origin(bk, g.lo[d], g.top[d], g.nin[d], g.split[d]); }

// the colour 0 .. 7 whose launch enumerates interior brick (b0, b1, b2): found from color_first, as the launches do
static int color_of(int b0, int b1, int b2)
{
    const int bk[3] = { b0, b1, b2 };
    int found = -1;
    for (int c = 0; c < 8; ++c) {
        bool all = true;
        for (int d = 0; d < 3; ++d) all = all && bk[d] >= color_first(c, d) && ((bk[d] - color_first(c, d)) & 1) == 0;
        if (all) { CHECK(found < 0, "brick %d %d %d in two colours", b0, b1, b2); found = c; }
    }
    CHECK(found >= 0, "brick %d %d %d in no colour", b0, b1, b2);
    return found;
}

// What a brick of order K WRITES are the BR + K slots per dim that its stencils reach; fresh_range reckons with whole boxes (BOX = BR + 3
// slots: the brick grid does not know the order), so for K < 3 it may call a slot overlapped that no earlier colour writes -- that slot
// keeps load + add + store, which is always correct.  Hence two coverings: `written` (BR + K) decides who the first writer is and that
// there is exactly one; `boxed` (BOX) is what fresh_range must reproduce exactly: fresh <=> no brick of an EARLIER colour holds the
// point in its box.  A fresh slot that its brick writes is then written by no earlier colour, and for K = 3 the two coverings agree:
// the first writer of every written point calls it fresh.

// one dim: every interior brick, every point its boxes cover (the boxes of the end bricks of a folding dim leave the lattice)
static void check_1d(int K, int n, bool fold)
{
    BrickGrid g;
    for (int d = 0; d < 3; ++d) brick_grid_dim(g, d, K, n, fold);
    const int d = 1;                                                  // (any dim: the other two sit at the first brick, bit 0)
    if (g.nin[d] <= 0) return;
    // bricks hold their cells: brick_and_cell and brick_origin agree
    for (int ft = g.lo[d]; ft < g.top[d]; ++ft) {
        const int bc = brick_and_cell(ft, g.lo[d], g.top[d], g.nin[d], g.split[d]);
        CHECK(origin(g, d, bc & 0xffff) + (bc >> 16) == ft, "K %d n %d fold %d cell %d", K, n, (int)fold, ft);
    }
    const int x0 = origin(g, d, NLO), x1 = origin(g, d, NLO + g.nin[d] - 1) + BOX;
    for (int x = x0; x < x1; ++x) {
        int owner = -1, best = 99, same = 0, boxed_best = 99, k_min = 1 << 30, k_max = -1;
        for (int bk = NLO; bk < NLO + g.nin[d]; ++bk) {
            const int o = origin(g, d, bk);
            if (x < o || x >= o + BOX) continue;
            k_min = bk < k_min ? bk : k_min; k_max = bk > k_max ? bk : k_max;
            const int c = color_of(NLO, bk, NLO);
            boxed_best = c < boxed_best ? c : boxed_best;
            if (x >= o + BR + K) continue;                            // (in the box, but not written)
            if (c < best) { best = c; owner = bk; same = 1; } else if (c == best) ++same;
        }
        CHECK(k_max >= 0, "K %d n %d fold %d: point %d inside the boxes' hull lies in none", K, n, (int)fold, x);
        CHECK(owner < 0 || same == 1, "K %d n %d fold %d: point %d has %d first writers of one colour", K, n, (int)fold, x, same);
        int nfresh = 0;
        for (int bk = k_min; bk <= k_max; ++bk) {
            const int o = origin(g, d, bk);
            if (x < o || x >= o + BOX) continue;
            int f_lo, f_hi;
            fresh_range(bk, d, g, f_lo, f_hi);
            CHECK(f_lo >= 0 && f_hi <= BOX, "range %d %d", f_lo, f_hi);
            const int slot = x - o, c = color_of(NLO, bk, NLO);
            const bool fresh = slot >= f_lo && slot < f_hi;
            CHECK(fresh == (c == boxed_best), "K %d n %d fold %d: point %d, brick %d slot %d: fresh %d [%d, %d), first colour of the boxes there %d", K, n, (int)fold, x, bk, slot, (int)fresh, f_lo, f_hi, boxed_best);
            if (fresh && slot < BR + K) { ++nfresh; CHECK(bk == owner, "K %d n %d fold %d: point %d: brick %d writes it fresh, first writer %d", K, n, (int)fold, x, bk, owner); }
        }
        CHECK(nfresh <= 1 && (K < 3 || owner < 0 || nfresh == 1), "K %d n %d fold %d: point %d: %d fresh writers, first writer %d", K, n, (int)fold, x, nfresh, owner);
    }
    // bricks_over names exactly the bricks whose box holds a lattice point
    for (int x = 0; x < n; ++x) {
        int k_lo, k_hi;
        bricks_over(x, d, g, k_lo, k_hi);
        for (int bk = NLO; bk < NLO + g.nin[d]; ++bk) {
            const bool covers = x >= origin(g, d, bk) && x < origin(g, d, bk) + BOX;
            CHECK(covers == (bk >= k_lo && bk <= k_hi), "K %d n %d fold %d: bricks_over(%d) = %d .. %d, brick %d covers %d", K, n, (int)fold, x, k_lo, k_hi, bk, (int)covers);
        }
    }
}

// three dims on one small lattice, every interior brick and every slot of its box
static void check_3d(int K, const int *n, const bool *fold)
{
    BrickGrid g;
    for (int d = 0; d < 3; ++d) brick_grid_dim(g, d, K, n[d], fold[d]);
    int x0[3], ext[3];
    for (int d = 0; d < 3; ++d) { x0[d] = origin(g, d, NLO); ext[d] = origin(g, d, NLO + g.nin[d] - 1) + BOX - x0[d]; }
    std::vector<int> best((size_t)ext[0] * ext[1] * ext[2], 99), count(best.size(), 0), boxed_best(best.size(), 99), nfresh(best.size(), 0);
    for (int pass = 0; pass < 2; ++pass)
        for (int b0 = NLO; b0 < NLO + g.nin[0]; ++b0) for (int b1 = NLO; b1 < NLO + g.nin[1]; ++b1) for (int b2 = NLO; b2 < NLO + g.nin[2]; ++b2) {
            const int c = color_of(b0, b1, b2), bk[3] = { b0, b1, b2 };
            int o[3], fl[3], fh[3];
            for (int d = 0; d < 3; ++d) { o[d] = origin(g, d, bk[d]) - x0[d]; fresh_range(bk[d], d, g, fl[d], fh[d]); }
            for (int i = 0; i < BOX; ++i) for (int j = 0; j < BOX; ++j) for (int k = 0; k < BOX; ++k) {
                const size_t at = ((size_t)(o[0] + i) * ext[1] + (o[1] + j)) * ext[2] + (o[2] + k);
                const bool written = i < BR + K && j < BR + K && k < BR + K;
                if (pass == 0) {
                    boxed_best[at] = c < boxed_best[at] ? c : boxed_best[at];
                    if (!written) continue;
                    if (c < best[at]) { best[at] = c; count[at] = 1; } else if (c == best[at]) ++count[at];
                } else {
                    const bool f = i >= fl[0] && i < fh[0] && j >= fl[1] && j < fh[1] && k >= fl[2] && k < fh[2];
                    CHECK(f == (c == boxed_best[at]), "3-D K %d: brick %d %d %d (colour %d) slot %d %d %d: fresh %d, first colour of the boxes there %d", K, b0, b1, b2, c, i, j, k, (int)f, boxed_best[at]);
                    if (f && written) { ++nfresh[at]; CHECK(c == best[at], "3-D K %d: brick %d %d %d (colour %d) writes slot %d %d %d fresh, first writer's colour %d", K, b0, b1, b2, c, i, j, k, best[at]); }
                }
            }
        }
    for (size_t at = 0; at < best.size(); ++at) {
        CHECK(boxed_best[at] < 8, "3-D K %d: point %zu inside the hull lies in no box", K, at);
        CHECK(best[at] == 99 || count[at] == 1, "3-D K %d: point %zu has %d first writers", K, at, count[at]);
        CHECK(nfresh[at] <= 1 && (K < 3 || best[at] == 99 || nfresh[at] == 1), "3-D K %d: point %zu: %d bricks write it fresh", K, at, nfresh[at]);
    }
}

int main()
{
    for (int fold = 0; fold < 2; ++fold)
        for (int K = 1; K <= 3; ++K)
            for (int n = 32; n <= 120; ++n) check_1d(K, n, fold != 0);
    // n = 84: a short brick of exactly K = 3 cells at `split`; n = 83: brick_grid drops the short brick (tests/test_first_writer_flush.py)
    {
        BrickGrid g;
        brick_grid_dim(g, 0, 3, 84, true);
        CHECK(origin(g, 0, NLO + g.split[0] + 1) - origin(g, 0, NLO + g.split[0]) == 3, "n = 84: short brick of %d cells", origin(g, 0, NLO + g.split[0] + 1) - origin(g, 0, NLO + g.split[0]));
        const int nin84 = g.nin[0];
        brick_grid_dim(g, 0, 3, 83, true);
        CHECK(g.nin[0] == nin84 - 1 && g.top[0] - g.lo[0] == BR * g.nin[0], "n = 83: %d bricks over %d cells", g.nin[0], g.top[0] - g.lo[0]);
    }
    const int n3[3] = { 84, 40, 53 };
    const bool f3[3] = { true, false, true };
    for (int K = 1; K <= 3; ++K) check_3d(K, n3, f3);
    const bool f3b[3] = { false, true, true };
    check_3d(3, n3, f3b);
    std::printf("ok %ld checks\n", checks);
    return 0;
}
