// amvs_strip_order.h -- block index -> (job, strip row, strip column) of the sweep step kernels, in one
// host + device function (the host copy is what tests/test_strip_order.py enumerates through
// amvs_sweep_order; no HIP header is needed to compile it).
#pragma once

#if defined(__HIPCC__)
#define AMVS_HD __host__ __device__ inline
#else
#define AMVS_HD inline
#endif

namespace amvs {

// Blocks are dealt round-robin to the 8 XCDs; xcd_remap hands every XCD a CONTIGUOUS range of work items
// (workgroups), walked in the order its blocks are dispatched.  Bijective.
AMVS_HD void xcd_range(int xcd, int nblk, int &lo, int &hi)
{
    const int q = nblk >> 3, r = nblk & 7;
    lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    hi = lo + q + (xcd < r ? 1 : 0);
}

AMVS_HD int xcd_remap(int bid, int nblk)
{
    int lo, hi;
    xcd_range(bid & 7, nblk, lo, hi);
    return lo + (bid >> 3);
}

AMVS_HD int order_ceil_div(int a, int b) { return (a + b - 1) / b; }

// Edge-first order inside an XCD's range [lo, hi) of work items.  A workgroup's duration grows from the image
// centre to its top and bottom edge (the gathers of the oblique sources touch 8 lines per row at the centre, ~30
// at the edges), and the workgroups dispatched LAST form the tail of the launch.  So the
// part of a view (band-major: of the launch) in the upper half of the image keeps its order -- walked DOWN, edge
// to centre -- and the part in the lower half is walked UP: item w of the lower part [m, e) becomes m + e - 1 - w.
// Which items an XCD owns does not change (its L2 footprint is the same), only when it starts each of them.
//   G     strips (paired: 2 x 2 strip units) per work item
//   rows  band rows (paired: pair rows) of a view, `cols` items-worth of columns per row in units
// An odd middle row counts to the upper half; a work item that straddles two rows / views belongs where its
// first unit lies.
AMVS_HD int edge_first_item(int w, int lo, int hi, int G, int rows, int cols, int n_jobs, int band_major)
{
    const int mrow = (rows + 1) / 2;                           // first row of the lower half
    int s, e, m;
    if (band_major) {
        s = lo; e = hi;
        m = order_ceil_div(mrow * n_jobs * cols, G);
    } else {
        const int T = rows * cols;
        const int job = (w * G) / T;
        s = order_ceil_div(job * T, G);
        e = order_ceil_div((job + 1) * T, G);
        m = order_ceil_div(job * T + mrow * cols, G);
    }
    if (s < lo) s = lo;
    if (e > hi) e = hi;
    if (m < s) m = s;
    if (m > e) m = e;
    return w < m ? w : m + (e - 1 - w);
}

// The strip of wave `wv` of block `bid` (of `nblk`) of a sweep step launch.  Classic: a block is `wg_waves`
// consecutive strips of the strip order (view-major, or band-major: band by band over all views); paired: a block
// is pair_cols strip columns x 2 vertically adjacent bands, `up` = 1 for the waves of the lower band, `paired` = 0
// for an odd last band that has no partner.  Returns false for a wave without a strip.
struct StripPos { int job, ty, tx, up, paired; };

AMVS_HD bool strip_decode(int n_jobs, int tiles_x, int tiles_y, int band_major, int pair, int pair_cols, int wg_waves,
                          int edge_first, int bid, int nblk, int wv, StripPos &p)
{
    int lo, hi;
    xcd_range(bid & 7, nblk, lo, hi);
    int w = lo + (bid >> 3);
    p.up = 0; p.paired = 0;
    if (pair) {
        const int col_pairs = (tiles_x + pair_cols - 1) / pair_cols, pair_rows = (tiles_y + 1) / 2;
        if (edge_first) w = edge_first_item(w, lo, hi, 1, pair_rows, col_pairs, n_jobs, 0);
        p.job = w / (col_pairs * pair_rows);
        const int rem = w - p.job * (col_pairs * pair_rows);
        const int py = rem / col_pairs, px = rem - py * col_pairs;
        p.tx = pair_cols * px + (wv % pair_cols);
        p.up = wv / pair_cols;
        p.ty = 2 * py + p.up;
        p.paired = 2 * py + 1 < tiles_y;
        return p.job < n_jobs && p.tx < tiles_x && p.ty < tiles_y;
    }
    if (edge_first) w = edge_first_item(w, lo, hi, wg_waves, tiles_y, tiles_x, n_jobs, band_major);
    const int t = w * wg_waves + wv;
    if (t >= n_jobs * tiles_x * tiles_y) return false;         // last workgroup only
    if (band_major) {
        const int per_band = n_jobs * tiles_x;
        p.ty = t / per_band;
        const int rem = t - p.ty * per_band;
        p.job = rem / tiles_x;
        p.tx = rem - p.job * tiles_x;
    } else {
        const int tiles_per_job = tiles_x * tiles_y;
        p.job = t / tiles_per_job;
        const int rem = t - p.job * tiles_per_job;
        p.ty = rem / tiles_x;
        p.tx = rem - p.ty * tiles_x;
    }
    return true;
}

}  // namespace amvs
