"""NumPy restatement of amvs_tsdf_fill, written from the definition in include/amvs.h and not from the kernel
(csrc/amvs_mesh_fill.hip): float32 at every operation, in the header's order, so that the device volume, the
generations and the counts can be compared bit for bit.  A helper module, not a conftest; no GPU.

Arrays are indexed [k, j, i] (x fastest, as on the device): tsdf and weight (nz, ny, nx), colour sums (nz, ny, nx, 3).

    fill        the vectorised statement: per step six shifted views of the state before the step, np.where at every
                accumulation so that no value of a neighbour that is not known reaches a result
    fill_loop   the same definition as a plain triple loop over the points with its own neighbour walk; the CPU tests
                hold `fill` to it on every small case
    VARIANTS    named near-misses of the definition (for `fill_loop`), each of which the CPU tests show to change some
                case of the family
"""
import numpy as np

F32 = np.float32

# the header's neighbour order (i-1), (i+1), (j-1), (j+1), (k-1), (k+1) as (axis of the [k, j, i] arrays, step)
NEIGHBOURS = ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1))


def _neighbour_view(a, axis, step, blank):
    """out[p] = a[p + step along axis] where that neighbour is in the grid, else `blank`."""
    out = np.full_like(a, blank)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if step > 0:
        src[axis], dst[axis] = slice(1, n), slice(0, n - 1)
    else:
        src[axis], dst[axis] = slice(0, n - 1), slice(1, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def fill(tsdf, weight, color_sum, steps, min_neighbours=1):
    """Returns tsdf, weight, colour sums (copies), gen (uint8) and the per-step counts (list of int)."""
    tsdf = np.array(tsdf, F32)
    weight = np.array(weight, F32)
    color = np.array(color_sum, F32)
    gen = (weight > 0).astype(np.uint8)
    counts = []
    for s in range(1, steps + 1):
        c = np.zeros(tsdf.shape, np.int32)
        acc = np.zeros(tsdf.shape, F32)
        cacc = np.zeros(color.shape, F32)
        for axis, step in NEIGHBOURS:
            g = _neighbour_view(gen, axis, step, 0)
            known = (g >= 1) & (g <= s)
            t = np.where(known, _neighbour_view(tsdf, axis, step, 0), F32(0))
            w = np.where(known, _neighbour_view(weight, axis, step, 1), F32(1))
            col = np.where(known[..., None], _neighbour_view(color, axis, step, 0), F32(0))
            acc = np.where(known, acc + t, acc)
            cacc = np.where(known[..., None], cacc + col / w[..., None], cacc)
            c += known
        take = (gen == 0) & (c >= min_neighbours)
        fc = np.where(take, c, 1).astype(F32)
        tsdf = np.where(take, acc / fc, tsdf)
        color = np.where(take[..., None], cacc / fc[..., None], color)
        weight = np.where(take, F32(1), weight)
        gen = np.where(take, np.uint8(s + 1), gen)
        counts.append(int(take.sum()))
        assert tsdf.dtype == F32 and color.dtype == F32 and weight.dtype == F32 and gen.dtype == np.uint8
    return tsdf, weight, color, gen, counts


# near-misses of the definition
VARIANTS = ("order", "divide_by_6", "colour_not_divided", "gauss_seidel", "no_lower_bound", "weight_left")


def fill_loop(tsdf, weight, color_sum, steps, min_neighbours=1, variant=None, stats=None):
    with np.errstate(all="ignore"):                 # the near-misses read garbage and divide by weight 0
        return _fill_loop(tsdf, weight, color_sum, steps, min_neighbours, variant, stats)


def _fill_loop(tsdf, weight, color_sum, steps, min_neighbours, variant, stats):
    """The definition point by point.  `variant`: None or one of VARIANTS.  `stats`, a dict, collects what the family's
    coverage is judged by: neighbour counts at filled and at refused points, reads of points filled earlier, lone -0.0f
    neighbours."""
    assert variant is None or variant in VARIANTS
    tsdf = np.array(tsdf, F32)
    weight = np.array(weight, F32)
    color = np.array(color_sum, F32)
    nz, ny, nx = tsdf.shape
    gen = np.zeros((nz, ny, nx), np.uint8)
    gen[weight > 0] = 1
    if stats is not None:
        stats.setdefault("filled_with", np.zeros(7, np.int64))
        stats.setdefault("refused_with", np.zeros(7, np.int64))
        stats.setdefault("from_filled", 0)
        stats.setdefault("lone_negative_zero", 0)
    walk = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]           # (di, dj, dk)
    if variant == "order":
        walk = walk[::-1]
    counts = []
    for s in range(1, steps + 1):
        if variant == "gauss_seidel":
            t_in, w_in, c_in, g_in = tsdf, weight, color, gen                               # sees this step's writes
        else:
            t_in, w_in, c_in, g_in = tsdf.copy(), weight.copy(), color.copy(), gen.copy()   # the state before the step
        done = 0
        g_list = g_in if variant == "gauss_seidel" else g_in.tolist()                     # plain ints: the walk is mostly this
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    if g_list[k][j][i] != 0:
                        continue
                    c = 0
                    acc = F32(0.0)
                    cacc = [F32(0.0), F32(0.0), F32(0.0)]
                    old = False
                    last = None
                    for di, dj, dk in walk:
                        a, b, d = i + di, j + dj, k + dk
                        if not (0 <= a < nx and 0 <= b < ny and 0 <= d < nz):
                            continue
                        gq = int(g_list[d][b][a])
                        if variant == "no_lower_bound":
                            known = gq <= s
                        elif variant == "gauss_seidel":
                            known = gq >= 1
                        else:
                            known = 1 <= gq <= s
                        if not known:
                            continue
                        c += 1
                        last = t_in[d, b, a]
                        old = old or gq >= 2
                        acc = F32(acc + t_in[d, b, a])
                        for ch in range(3):
                            mean = c_in[d, b, a, ch] if variant == "colour_not_divided" else F32(c_in[d, b, a, ch] / w_in[d, b, a])
                            cacc[ch] = F32(cacc[ch] + mean)
                    if c < min_neighbours:
                        if stats is not None:
                            stats["refused_with"][c] += 1
                        continue
                    fc = F32(6 if variant == "divide_by_6" else c)
                    tsdf[k, j, i] = F32(acc / fc)
                    for ch in range(3):
                        color[k, j, i, ch] = F32(cacc[ch] / fc)
                    if variant != "weight_left":
                        weight[k, j, i] = F32(1.0)
                    gen[k, j, i] = s + 1
                    done += 1
                    if stats is not None:
                        stats["filled_with"][c] += 1
                        stats["from_filled"] += int(old)
                        stats["lone_negative_zero"] += int(c == 1 and last == 0 and bool(np.signbit(last)))
        counts.append(done)
    return tsdf, weight, color, gen, counts
