// amvs_capi_features.hip -- the entry points of include/amvs_features.h: CLAHE, the resident SIFT scale space and the
// fetch of one of its levels, the keypoints and descriptors, their fetch and their way into a descriptor slot.  Parameter errors are reported before anything is allocated.
#include "amvs_ctx.h"
#include "../../include/amvs_features.h"
#include "../../include/amvs_match.h"

#include <cmath>

using namespace amvs::host;

static_assert(AMVS_SIFT_GAUSS == amvs::SIFT_GAUSS && AMVS_SIFT_DOG == amvs::SIFT_DOG && AMVS_SIFT_LAYERS == amvs::SIFT_LAYERS &&
                  AMVS_SIFT_MAX_RADIUS == amvs::SIFT_MAX_RADIUS,
              "include/amvs_features.h and the kernels' constants");

namespace {

const char *side_error(int h, int w, int min_side)
{
    if (h < min_side || w < min_side) return "image side below the minimum";
    if (h > AMVS_FEATURES_MAX_SIDE || w > AMVS_FEATURES_MAX_SIDE) return "image side above AMVS_FEATURES_MAX_SIDE";
    return nullptr;
}

// the scale space of a validated image into c->sift (NULL: the resident CLAHE result); synchronises
int build_space(amvs_ctx *c, const uint8_t *gray_host, int h, int w, double sigma)
{
    amvs::SiftState &s = c->sift;
    s.n_octaves = 0;
    const int n_oct = amvs::sift_octaves(h, w);            // <= 13 for a side of 8192
    size_t g_total = 0, d_total = 0;
    for (int o = 0; o < n_oct; ++o) {
        s.h[o] = o ? s.h[o - 1] / 2 : 2 * h;
        s.w[o] = o ? s.w[o - 1] / 2 : 2 * w;
        s.g_off[o] = g_total;
        s.d_off[o] = d_total;
        const size_t px = (size_t)s.h[o] * s.w[o];
        g_total += amvs::SIFT_GAUSS * px;
        d_total += amvs::SIFT_DOG * px;
    }
    double sig[6];
    amvs::sift_sigmas(sigma, sig);
    amvs::GaussTaps taps[6];
    for (int i = 0; i < 6; ++i) {
        taps[i] = amvs::sift_gauss_taps(sig[i]);
        if (taps[i].r > amvs::SIFT_MAX_RADIUS) return fail(c, AMVS_EINVAL, "blur radius above AMVS_SIFT_MAX_RADIUS");
    }

    const size_t px0 = (size_t)s.h[0] * s.w[0];
    amvs::ScratchCache::Lease src, up, tmp;
    HIPCHK(c, s.gauss.reserve(g_total, c->cache));
    HIPCHK(c, s.dog.reserve(d_total, c->cache));
    HIPCHK(c, c->cache.lease(up, px0 * sizeof(float)));
    HIPCHK(c, c->cache.lease(tmp, px0 * sizeof(float)));
    const unsigned char *d_gray = c->clahe.out.get();
    if (gray_host) {
        HIPCHK(c, c->cache.lease(src, (size_t)h * w));
        HIPCHK(c, hipMemcpyAsync(src.get(), gray_host, (size_t)h * w, hipMemcpyHostToDevice, c->stream));
        d_gray = src.get<unsigned char>();
    }
    HIPCHK(c, amvs::launch_sift_upsample(d_gray, h, w, up.get<float>(), c->stream));
    for (int o = 0; o < n_oct; ++o) {
        const size_t px = (size_t)s.h[o] * s.w[o];
        float *g = s.gauss.get() + s.g_off[o], *d = s.dog.get() + s.d_off[o];
        if (o == 0)
            HIPCHK(c, amvs::launch_sift_blur(up.get<float>(), s.h[0], s.w[0], taps[0], tmp.get<float>(), g, nullptr, nullptr, c->stream));
        else
            HIPCHK(c, amvs::launch_sift_halve(s.gauss.get() + s.g_off[o - 1] + amvs::SIFT_LAYERS * (size_t)s.h[o - 1] * s.w[o - 1],
                                              s.h[o - 1], s.w[o - 1], g, c->stream));
        for (int i = 1; i < amvs::SIFT_GAUSS; ++i)
            HIPCHK(c, amvs::launch_sift_blur(g + (i - 1) * px, s.h[o], s.w[o], taps[i], tmp.get<float>(), g + i * px, g + (i - 1) * px,
                                             d + (i - 1) * px, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    s.n_octaves = n_oct;
    return AMVS_OK;
}

// what amvs_sift_scale_space and amvs_sift_extract refuse alike; NULL = fine
const char *space_error(const amvs_ctx *c, const uint8_t *gray_host, int h, int w, double sigma)
{
    if (const char *why = side_error(h, w, AMVS_SIFT_MIN_SIDE)) return why;
    if (!std::isfinite(sigma) || sigma < AMVS_SIFT_MIN_SIGMA || sigma > AMVS_SIFT_MAX_SIGMA)
        return "sigma must be finite and within AMVS_SIFT_MIN_SIGMA .. AMVS_SIFT_MAX_SIGMA";
    if (!gray_host && (c->clahe.h != h || c->clahe.w != w || h == 0)) return "NULL image and no resident CLAHE result of this size";
    return nullptr;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int amvs_clahe_u8(amvs_ctx *c, const uint8_t *gray_host, int h, int w, float clip_limit, int grid_x, int grid_y, uint8_t *out_host)
{
    if (!c) return AMVS_EINVAL;
    if (!gray_host) return fail(c, AMVS_EINVAL, "NULL image");
    if (const char *why = side_error(h, w, 1)) return fail(c, AMVS_EINVAL, why);
    if (grid_x < 1 || grid_y < 1 || grid_x > AMVS_CLAHE_MAX_GRID || grid_y > AMVS_CLAHE_MAX_GRID)
        return fail(c, AMVS_EINVAL, "grid outside 1 .. AMVS_CLAHE_MAX_GRID");
    if (!std::isfinite(clip_limit) || clip_limit < 0.0f) return fail(c, AMVS_EINVAL, "clip_limit must be finite and not negative");
    int rc = bind_device(c);
    if (rc) return rc;
    const int tw = (w + grid_x - 1) / grid_x, th = (h + grid_y - 1) / grid_y, area = tw * th;
    int limit = 0;                                         // 0: the clipping is off
    if (clip_limit != 0.0f) {
        const float t = (clip_limit * (float)area) / 256.0f;
        if (!(t >= (float)area)) limit = (int)t > 1 ? (int)t : 1;
    }
    const size_t n = (size_t)h * w;
    amvs::ScratchCache::Lease src, lut;
    HIPCHK(c, c->cache.lease(src, n));
    HIPCHK(c, c->cache.lease(lut, (size_t)grid_x * grid_y * 256));
    c->clahe.h = c->clahe.w = 0;
    HIPCHK(c, c->clahe.out.reserve(n, c->cache));
    HIPCHK(c, hipMemcpyAsync(src.get(), gray_host, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, amvs::launch_clahe_luts(src.get<unsigned char>(), h, w, grid_x, grid_y, limit, lut.get<unsigned char>(), c->stream));
    HIPCHK(c, amvs::launch_clahe_apply(src.get<unsigned char>(), h, w, grid_x, grid_y, lut.get<unsigned char>(), c->clahe.out.get(),
                                       c->stream));
    if (out_host) HIPCHK(c, hipMemcpyAsync(out_host, c->clahe.out.get(), n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->clahe.h = h;
    c->clahe.w = w;
    return checked(c, AMVS_OK);
}

int amvs_sift_scale_space(amvs_ctx *c, const uint8_t *gray_host, int h, int w, double sigma, int *n_octaves)
{
    if (!c) return AMVS_EINVAL;
    if (!n_octaves) return fail(c, AMVS_EINVAL, "NULL n_octaves");
    if (const char *why = space_error(c, gray_host, h, w, sigma)) return fail(c, AMVS_EINVAL, why);
    int rc = bind_device(c);
    if (rc) return rc;
    c->sift.n_kp = -1;
    rc = build_space(c, gray_host, h, w, sigma);
    if (rc) return rc;
    *n_octaves = c->sift.n_octaves;
    return checked(c, AMVS_OK);
}

int amvs_sift_extract(amvs_ctx *c, const uint8_t *gray_host, int h, int w, int n_features, float contrast_threshold, float edge_threshold,
                      double sigma, int *n_keypoints)
{
    if (!c) return AMVS_EINVAL;
    if (!n_keypoints) return fail(c, AMVS_EINVAL, "NULL n_keypoints");
    if (n_features < 0 || n_features > AMVS_SIFT_MAX_FEATURES) return fail(c, AMVS_EINVAL, "n_features outside 0 .. AMVS_SIFT_MAX_FEATURES");
    if (!std::isfinite(contrast_threshold) || contrast_threshold < 0.0f)
        return fail(c, AMVS_EINVAL, "contrast_threshold must be finite and not negative");
    if (!std::isfinite(edge_threshold) || !(edge_threshold > 0.0f)) return fail(c, AMVS_EINVAL, "edge_threshold must be finite and positive");
    if (const char *why = space_error(c, gray_host, h, w, sigma)) return fail(c, AMVS_EINVAL, why);
    int rc = bind_device(c);
    if (rc) return rc;
    c->sift.n_kp = -1;
    rc = build_space(c, gray_host, h, w, sigma);
    if (rc) return rc;
    amvs::SiftParams prm;
    prm.pre_threshold = (float)std::floor(0.5 * (double)contrast_threshold / 3.0 * 255.0);
    prm.contrast_threshold = contrast_threshold;
    prm.edge_threshold = edge_threshold;
    prm.sigma = (float)sigma;
    bool too_many = false;
    HIPCHK(c, amvs::sift_keypoints(c->sift, prm, n_features, AMVS_SIFT_MAX_FEATURES, c->cache, &too_many, c->stream));
    if (too_many) return fail(c, AMVS_EINVAL, "more than AMVS_SIFT_MAX_FEATURES keypoints before the selection");
    *n_keypoints = c->sift.n_kp;
    return checked(c, AMVS_OK);
}

int amvs_sift_fetch(amvs_ctx *c, float *keypoints_out, uint8_t *descriptors_out, int n)
{
    if (!c) return AMVS_EINVAL;
    if (c->sift.n_kp < 0) return fail(c, AMVS_EINVAL, "no resident keypoints");
    if (n != c->sift.n_kp) return fail(c, AMVS_EINVAL, "n is not the resident keypoint count");
    if (n == 0 || (!keypoints_out && !descriptors_out)) return AMVS_OK;
    int rc = bind_device(c);
    if (rc) return rc;
    if (keypoints_out)
        HIPCHK(c, hipMemcpyAsync(keypoints_out, c->sift.kp.get(), (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (descriptors_out)
        HIPCHK(c, hipMemcpyAsync(descriptors_out, c->sift.desc.get(), (size_t)n * 128, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sift_to_slot(amvs_ctx *c, int slot)
{
    if (!c) return AMVS_EINVAL;
    if (c->sift.n_kp < 0) return fail(c, AMVS_EINVAL, "no resident keypoints");
    if (slot < 0 || slot >= AMVS_DESC_MAX_SLOTS) return fail(c, AMVS_EINVAL, "slot outside 0 .. AMVS_DESC_MAX_SLOTS - 1");
    if (c->sift.n_kp > AMVS_DESC_MAX_ROWS) return fail(c, AMVS_EINVAL, "more keypoints than AMVS_DESC_MAX_ROWS");
    int rc = bind_device(c);
    if (rc) return rc;
    HIPCHK(c, amvs::desc_set_device((const unsigned char *)c->sift.desc.get(), c->sift.n_kp, c->cache, c->desc[slot], c->stream));
    return checked(c, AMVS_OK);
}

int amvs_sift_fetch_level(amvs_ctx *c, int octave, int index, int dog, float *out_host, int *h_out, int *w_out)
{
    if (!c) return AMVS_EINVAL;
    const amvs::SiftState &s = c->sift;
    if (s.n_octaves < 1) return fail(c, AMVS_EINVAL, "no resident scale space");
    if (octave < 0 || octave >= s.n_octaves) return fail(c, AMVS_EINVAL, "octave outside the scale space");
    if (index < 0 || index >= (dog ? amvs::SIFT_DOG : amvs::SIFT_GAUSS)) return fail(c, AMVS_EINVAL, "index outside the octave");
    if (h_out) *h_out = s.h[octave];
    if (w_out) *w_out = s.w[octave];
    if (!out_host) return AMVS_OK;
    int rc = bind_device(c);
    if (rc) return rc;
    const size_t px = (size_t)s.h[octave] * s.w[octave];
    const float *p = (dog ? s.dog.get() + s.d_off[octave] : s.gauss.get() + s.g_off[octave]) + (size_t)index * px;
    HIPCHK(c, hipMemcpyAsync(out_host, p, px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return checked(c, AMVS_OK);
}

}  // extern "C"
#pragma GCC visibility pop
