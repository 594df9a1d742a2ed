// rtdd_harness -- headless stand-in for the reference's interactive shell (/root/reference/src/main.cpp).
//
// main.cpp is an OpenCV HighGUI event loop over cv::cuda::GpuMat and cannot be built on a ROCm box
// (SURVEY.md section 0); this program makes the SAME sequence of calls through librtdd.so's C ABI
// with plain files instead of windows:
//     -i image.jpg  -a annotation.png      (main.cpp:81-90; JPEG (jpeg_reader.hpp: libjpeg's default decode, restated), 8-bit PNG, binary PPM / PGM)
//     key 'd'  -> one depth estimate        (main.cpp:232-295)  -> <out>DepthMap.pgm     (main.cpp:306-310)
//     key 's'  -> also the annotated image   (main.cpp:298-303)  -> <out>AnnotatedImage.ppm: the image with the scribbles painted in
//     key 'b'/'g'/'h' -> --effect defocus|desaturation|haze     -> <out>ArtisticEffect.ppm (main.cpp:190-230, 312-316)
//     extensions: --effect refocus [--focus D | --focus-at X,Y] [--aperture A] [--bokeh box|disc|spread]   (rtdd_simulate_refocus; default: focus depth 0,
//                 aperture 0.025 = the defocus; --bokeh disc: rtdd_simulate_lens_blur's round aperture; --bokeh spread: rtdd_simulate_bokeh, the occlusion-aware blur), --effect haze [--haze-beta B] [--airlight b,g,r]   (rtdd_simulate_haze_ex when either is given),
//                 --effect stereo --disparity D [--zero-parallax Z | --zero-parallax-at X,Y] [--anaglyph]   (rtdd_simulate_stereo; default:
//                 zero parallax at depth 0, the view),
//                 --effect parallax --shift dx,dy [--dolly z] [--zero-parallax Z | --zero-parallax-at X,Y]   (rtdd_simulate_parallax: the camera moved
//                 sideways, up or forward; default: no dolly, zero parallax at depth 0; with --plate-region id [--remove-grow N] [--remove-behind D]
//                 the painted region `id` is removed into a background plate held aside (rtdd_remove_object; the scene stays) and the view
//                 rendered over both layers (rtdd_simulate_parallax_layered); --parallax-depth-out FILE and --parallax-coverage FILE write
//                 the view's depth map (u8, as DepthMap) and its coverage codes as PGM or PNG),
//                 --effect relight [--light-dir x,y,z | --light-at X,Y [--light-height H] [--light-radius R]] [--relief S] [--ambient A] [--diffuse D]
//                 [--light-color b,g,r]   (rtdd_simulate_relight; default: a white directional light from the upper left, (-1, -1, 1), relief 2,
//                 ambient 0.25, diffuse 1; --light-at: a point light over that pixel, anchored at its depth, height 100, radius 200)
//                 --effect relight --shadows N [--shadow-bias B] [--shadow-softness S] [--shadow-strength T]   (rtdd_simulate_relight_shadowed: cast
//                 shadows, N steps of the march; default bias 0, softness 0 = hard, strength 1)
//                 --effect ao [--ao-radius R] [--ao-directions 4|8] [--ao-bias B] [--ao-strength T] [--relief S] [--ao-map]   (rtdd_simulate_ambient_occlusion
//                 without a light: the original darkened in creases, or --ao-map: the occlusion as a gray map; default radius 16, 8 directions,
//                 bias 0, strength 1, relief 2), --effect relight --ao R [--ao-directions ..] [--ao-bias ..] [--ao-strength ..]   (the same call
//                 under relight's light: its ambient term occluded; not together with --shadows)
//                 --effect lighting [relight's light flags] [--shadows N] [--shadow-bias ..] [--shadow-softness ..] [--shadow-strength ..] [--ao R]
//                 [--ao-directions ..] [--ao-bias ..] [--ao-strength ..]   (rtdd_simulate_lighting: shade, cast shadows and the occluded ambient
//                 term in one call; default 256 steps, radius 16)
//     key 't'  -> prints "Processing Time"  (main.cpp:320-322; wall clock here, the reference uses clock()); the process's one-time costs
//                 (~20 ms: code objects, first allocations) are paid by a warm-up on a context of its own first -- --cold leaves it out
//     --paint x,y,label,radius  = a mouse drag sample (main.cpp:46-62), repeatable; --paint-at F:x,y,label,radius = the same while --live
//                                 runs, in front of frame F (the user painting into a live view)
//     --refine sor|mg|auto [--tolerance T] = extension: converge the finest level after the estimate (rtdd_refine_depth)
//     --edges gray|color = extension: the estimates' edge weights from the gray image (default, the reference's) or from the BGR image (rtdd_pyramid_set_guide)
//     --regions cut|smooth|both = extension: depth regions (rtdd_pyramid_set_regions) -- the estimates cut the edges between different region
//                                 ids, smooth the edges inside one region, or both; the regions are painted into the pyramid's region pair
//                                 before the estimate by --region-fill "x,y;x,y;...:id" (a lasso, rtdd_fill_polygon under the --fill-rule in
//                                 force) and --region-wand "x,y,tol:id" (a click, rtdd_fill_similar on the photograph under the
//                                 --wand-connect in force), the fills first, each kind in command-line order; AFTER the estimate by
//                                 --region-surface "x,y,step[,below,above]:id" (a click on the estimated depth map, rtdd_fill_surface;
//                                 behind --surface-global every pixel in the band), which also fills the level-0 code plane again, so
//                                 that --remove-region / --move-region / --plate-region take the region; not with --live or --batch
//     --segment "step[,lo,hi[,minPixels[,maxRegions[,firstCode]]]]" = extension, with --regions: every surface of the estimated depth map at
//                                 once (rtdd_segment_surfaces; defaults 0,255, 64, 8, 1) -- the largest become the regions firstCode,
//                                 firstCode + 1, ... of the region pair, one line printed per region; behind the --region-surface clicks,
//                                 and like them it fills the level-0 code plane again; not with --live or --batch
//     --layer sprite --layer-alpha alpha --layer-at x,y [--layer-scale S] [--layer-filter nearest|bilinear] [--layer-depth z | --layer-plane
//                                 x0,y0,z0,x1,y1,z1] [--layer-feather f] [--layer-opacity o] = extension: a sprite inserted into the scene at
//                                 a depth (rtdd_composite_layer), after the estimate and before --effect, which then runs on the composite and
//                                 ITS depth map; without --effect <out>ArtisticEffect is the composite; not with --live
//     --remove-region id [--remove-grow N] [--remove-behind D] = extension: the painted region `id` (--regions, --region-fill / --region-wand)
//                                 taken out of the scene after the estimate (rtdd_remove_object; the mask is the region's code plane): the
//                                 hole, grown by N, is filled from the pixels at least D far.  --move-region id:dx,dy[:depth] lifts the
//                                 region (rtdd_lift_layer), removes it and composites it (dx, dy) away at `depth` (default: its own nearest
//                                 depth, one constant).  Before --layer and --effect, which run on the result and ITS depth map; without
//                                 them <out>ArtisticEffect is the result; not with --live
//     --select-grow R2 | --select-shrink R2 = extension, with --remove-region, --move-region or --plate-region: the region's code plane is
//                                 first refined into a 0 / 255 mask (rtdd_refine_mask: grown out to, or shrunk in by, the squared Euclidean
//                                 distance R2, 1 .. 1048576), and that mask is what the removal, the lift and the plate read; one of the two
//     --move-feather W          = extension, with --move-region: the sprite gets a soft edge, W pixels wide (0 < W <= 64), inside the selection
//                                 (rtdd_refine_mask's feather lo = -W, hi = 0, then rtdd_lift_layer_matte); the removal stays on the hard mask
// and adds what the reference cannot do: --devices N --batch B runs B independent estimates
// round-robin over N GPUs, one host thread + one HIP stream + one rtdd_ctx per GPU, no collective.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <zlib.h>

#include "rtdd.h"
#include "jpeg_reader.hpp"

struct Pnm { int w = 0, h = 0, ch = 0; std::vector<unsigned char> px; };

static bool read_pnm(const std::string &path, Pnm &im) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[3] = {0, 0, 0};
    int maxv = 0;
    auto skip = [&]() { int c; while ((c = std::fgetc(f)) != EOF) { if (c == '#') { while ((c = std::fgetc(f)) != EOF && c != '\n') {} } else if (c > ' ') { std::ungetc(c, f); break; } } };
    if (std::fscanf(f, "%2s", magic) != 1) { std::fclose(f); return false; }
    im.ch = !std::strcmp(magic, "P6") ? 3 : (!std::strcmp(magic, "P5") ? 1 : 0);
    if (!im.ch) { std::fclose(f); return false; }
    skip(); if (std::fscanf(f, "%d", &im.w) != 1) { std::fclose(f); return false; }
    skip(); if (std::fscanf(f, "%d", &im.h) != 1) { std::fclose(f); return false; }
    skip(); if (std::fscanf(f, "%d", &maxv) != 1 || maxv != 255) { std::fclose(f); return false; }
    std::fgetc(f);
    if (im.w <= 0 || im.h <= 0 || im.w > 65535 || im.h > 65535) { std::fclose(f); return false; }
    const long at = std::ftell(f);
    std::fseek(f, 0, SEEK_END);
    const long left = std::ftell(f) - at;                          // (a header must not make us allocate what the file cannot hold)
    std::fseek(f, at, SEEK_SET);
    if (at < 0 || left < 0 || (unsigned long long)left < (unsigned long long)im.w * im.h * im.ch) { std::fclose(f); return false; }
    im.px.resize((size_t)im.w * im.h * im.ch);
    const bool ok = std::fread(im.px.data(), 1, im.px.size(), f) == im.px.size();
    std::fclose(f);
    return ok;
}

static bool write_pnm(const std::string &path, int w, int h, int ch, const unsigned char *px) {
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "%s\n%d %d\n255\n", ch == 3 ? "P6" : "P5", w, h);
    const bool ok = std::fwrite(px, 1, (size_t)w * h * ch, f) == (size_t)w * h * ch;
    std::fclose(f);
    return ok;
}

// ---- PNG (the dataset's annotations are PNG, src/main.cpp:158-161; the reference saves PNG, :312-316) on zlib alone -----------
// Reader: 8-bit, non-interlaced, gray / gray+alpha / RGB / RGBA / palette; alpha is dropped.  Writer: 8-bit gray or RGB, filter 0.
static uint32_t be32(const unsigned char *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

static bool read_png(const std::string &path, Pnm &im) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::vector<unsigned char> file;
    unsigned char buf[65536]; size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
    std::fclose(f);
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    if (file.size() < 8 || std::memcmp(file.data(), sig, 8)) return false;
    int depth = 0, ctype = -1, interlace = 0;
    std::vector<unsigned char> idat, plte;
    for (size_t p = 8; p + 12 <= file.size();) {
        const uint32_t len = be32(&file[p]);
        if (p + 12 + len > file.size()) return false;
        const char *type = (const char *)&file[p + 4];
        const unsigned char *data = &file[p + 8];
        if (!std::memcmp(type, "IHDR", 4) && len >= 13) { im.w = (int)be32(data); im.h = (int)be32(data + 4); depth = data[8]; ctype = data[9]; interlace = data[12]; }
        else if (!std::memcmp(type, "PLTE", 4)) plte.assign(data, data + len);
        else if (!std::memcmp(type, "IDAT", 4)) idat.insert(idat.end(), data, data + len);
        else if (!std::memcmp(type, "IEND", 4)) break;
        p += 12 + len;
    }
    const int spp = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;      // samples per pixel in the file
    if (depth != 8 || !spp || interlace || im.w <= 0 || im.h <= 0 || im.w > 65535 || im.h > 65535) return false;
    const size_t stride = (size_t)im.w * spp;
    // (deflate expands by at most ~1032 : 1: a header that promises more than its IDAT can hold is refused before anything is allocated)
    if ((unsigned long long)(stride + 1) * im.h > (unsigned long long)idat.size() * 1100ull + 65536ull) return false;
    std::vector<unsigned char> raw((stride + 1) * im.h);
    uLongf rawlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &rawlen, idat.data(), (uLong)idat.size()) != Z_OK || rawlen != raw.size()) return false;
    std::vector<unsigned char> prev(stride, 0), cur(stride);
    im.ch = (ctype == 0 || ctype == 4) ? 1 : 3;
    im.px.resize((size_t)im.w * im.h * im.ch);
    for (int y = 0; y < im.h; y++) {
        const unsigned char *line = &raw[(stride + 1) * y];
        const int ft = line[0];
        for (size_t i = 0; i < stride; i++) {
            const int a = i >= (size_t)spp ? cur[i - spp] : 0, b = prev[i], c = i >= (size_t)spp ? prev[i - spp] : 0;
            int pred = 0;
            if (ft == 1) pred = a; else if (ft == 2) pred = b; else if (ft == 3) pred = (a + b) >> 1;
            else if (ft == 4) { const int pp = a + b - c, pa = std::abs(pp - a), pb = std::abs(pp - b), pc = std::abs(pp - c); pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            else if (ft != 0) return false;
            cur[i] = (unsigned char)(line[1 + i] + pred);
        }
        for (int x = 0; x < im.w; x++) {
            unsigned char *o = &im.px[((size_t)y * im.w + x) * im.ch];
            const unsigned char *s = &cur[(size_t)x * spp];
            if (ctype == 0 || ctype == 4) o[0] = s[0];
            else if (ctype == 3) { if ((size_t)s[0] * 3 + 2 >= plte.size()) return false; o[0] = plte[s[0] * 3]; o[1] = plte[s[0] * 3 + 1]; o[2] = plte[s[0] * 3 + 2]; }
            else { o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; }
        }
        prev.swap(cur);
    }
    return true;
}

static bool write_png(const std::string &path, int w, int h, int ch, const unsigned char *px) {
    std::vector<unsigned char> raw(((size_t)w * ch + 1) * h);
    for (int y = 0; y < h; y++) { raw[((size_t)w * ch + 1) * y] = 0; std::memcpy(&raw[((size_t)w * ch + 1) * y + 1], px + (size_t)y * w * ch, (size_t)w * ch); }
    uLongf clen = compressBound((uLong)raw.size());
    std::vector<unsigned char> comp(clen);
    if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), 6) != Z_OK) return false;
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    auto chunk = [&](const char *type, const unsigned char *data, uint32_t len) {
        unsigned char hdr[8] = {(unsigned char)(len >> 24), (unsigned char)(len >> 16), (unsigned char)(len >> 8), (unsigned char)len, (unsigned char)type[0], (unsigned char)type[1], (unsigned char)type[2], (unsigned char)type[3]};
        uLong crc = crc32(0L, hdr + 4, 4);
        if (len) crc = crc32(crc, data, len);
        const unsigned char tail[4] = {(unsigned char)(crc >> 24), (unsigned char)(crc >> 16), (unsigned char)(crc >> 8), (unsigned char)crc};
        std::fwrite(hdr, 1, 8, f); if (len) std::fwrite(data, 1, len, f); std::fwrite(tail, 1, 4, f);
    };
    static const unsigned char sig[8] = {137, 80, 78, 71, 13, 10, 26, 10};
    std::fwrite(sig, 1, 8, f);
    const unsigned char ihdr[13] = {(unsigned char)(w >> 24), (unsigned char)(w >> 16), (unsigned char)(w >> 8), (unsigned char)w, (unsigned char)(h >> 24), (unsigned char)(h >> 16), (unsigned char)(h >> 8), (unsigned char)h,
                                    8, (unsigned char)(ch == 3 ? 2 : 0), 0, 0, 0};
    chunk("IHDR", ihdr, 13); chunk("IDAT", comp.data(), (uint32_t)clen); chunk("IEND", nullptr, 0);
    return std::fclose(f) == 0;
}

static bool ends_with(const std::string &s, const char *suffix) { const size_t n = std::strlen(suffix); return s.size() >= n && !s.compare(s.size() - n, n, suffix); }
static bool read_jpeg(const std::string &path, Pnm &im) {           // (cv::imread's decode, restated: harness/jpeg_reader.hpp)
    std::string why;
    if (rtdd_jpeg::read_file(path, im.w, im.h, im.ch, im.px, &why)) return true;
    std::fprintf(stderr, "%s: %s\n", path.c_str(), why.c_str());
    return false;
}
static bool read_image(const std::string &path, Pnm &im) {
    if (ends_with(path, ".png")) return read_png(path, im);
    if (ends_with(path, ".jpg") || ends_with(path, ".jpeg") || ends_with(path, ".JPG") || ends_with(path, ".JPEG")) return read_jpeg(path, im);
    return read_pnm(path, im);
}
static bool write_image(const std::string &path, int w, int h, int ch, const unsigned char *px) { return ends_with(path, ".png") ? write_png(path, w, h, ch, px) : write_pnm(path, w, h, ch, px); }

#define CK(call) do { int rc_ = (call); if (rc_ != RTDD_OK) { std::printf("%s: %s (%s)\n", #call, rtdd_status_string(rc_), rtdd_last_error(ctx)); return rc_; } } while (0)

struct Paint { int x, y, label, radius, frame; };      // frame: --paint-at (live mode: in front of that frame); --paint: before the first estimate
struct LiveStroke { rtdd_ramp_stroke s; int frame; };   // --stroke-at / --erase-at / --ramp-at: in front of live frame `frame`
struct Job {
    Pnm bgr, ann;                 // bgr is BGR-interleaved like cv::imread's Mat
    bool has_ann = false;
    std::vector<Paint> paints, live_paints;
    // --stroke / --erase / --ramp, in command-line order, as ramp records (a constant stroke: label0 == label1): ONE call after the --paint
    // stamps -- rtdd_paint_ramp_strokes when a --ramp is among them, rtdd_paint_strokes otherwise
    std::vector<rtdd_ramp_stroke> strokes;
    bool has_ramp = false;
    std::vector<LiveStroke> live_strokes;
    // --fill / --fill-erase, in command-line order among themselves: one rtdd_fill_polygon call each, after the strokes' call
    struct Lasso { std::vector<int> xy; rtdd_fill fill; };
    std::vector<Lasso> fills;
    int fill_rule = RTDD_FILL_NONZERO;      // --fill-rule nonzero|evenodd: the rule of the --fill / --fill-erase flags behind it
    // --wand / --wand-erase, in command-line order among themselves: one rtdd_fill_similar call each, after the polygons; --wand-at /
    // --wand-erase-at (frame >= 0): in front of that live frame
    struct Wand { rtdd_wand w; int frame; };
    std::vector<Wand> wands, live_wands;
    int wand_flags = 0;                     // --wand-connect 4|8: the connectivity of the --wand flags behind it
    std::string effect;
    int iters = 1000;
    std::string refine;           // "" | "sor" | "mg": rtdd_refine_depth after every estimate
    float tolerance = 1e-4f;
    double aperture = 0.025;      // --effect refocus: --aperture, --focus / --focus-at (focus_x < 0: the depth focus_depth)
    float focus_depth = 0.0f;
    int focus_x = -1, focus_y = -1;
    bool disc = false;            // --bokeh disc: rtdd_simulate_lens_blur with the round aperture (box, the default: rtdd_simulate_refocus)
    bool spread = false;          // --bokeh spread: rtdd_simulate_bokeh, every pixel spread over its own disc
    bool haze_ex = false;         // --haze-beta / --airlight given: rtdd_simulate_haze_ex
    float haze_beta = 2.0f;
    int air[3] = {255, 255, 255}; // b, g, r
    int disparity = 0;            // --effect stereo: --disparity, --zero-parallax / --zero-parallax-at (zero_x < 0: the depth zero_depth), --anaglyph
    float zero_depth = 0.0f;
    int zero_x = -1, zero_y = -1;
    bool anaglyph = false;
    int shift_x = 0, shift_y = 0; // --effect parallax: --shift, --dolly, and stereo's --zero-parallax / --zero-parallax-at
    float dolly = 0.0f;
    // --effect relight: --light-dir (directional) or --light-at (a point light over that pixel, anchored at its depth), --light-height, --light-radius,
    // --relief, --ambient, --diffuse, --light-color
    rtdd_light light = {RTDD_LIGHT_DIRECTIONAL, -1.0f, -1.0f, 1.0f, 0.0f, -1, -1, 200.0f, 2.0f, 0.25f, 1.0f, 255, 255, 255};
    float light_height = 100.0f;
    // --shadows N (given: rtdd_simulate_relight_shadowed; --effect lighting: the steps of rtdd_simulate_lighting, 256 when not given), --shadow-bias,
    // --shadow-softness, --shadow-strength
    bool shadows = false;
    rtdd_shadow shadow = {0, 0.0f, 0.0f, 1.0f};
    // --effect ao, or --effect relight --ao R (ao_lit): rtdd_simulate_ambient_occlusion; --ao-radius / --ao R, --ao-directions, --ao-bias, --ao-strength,
    // --ao-map; the relief is --relief's (the light's)
    bool ao_lit = false;
    rtdd_ambient_occlusion ao = {RTDD_AO_SHADE, 8, 16, 2.0f, 0.0f, 1.0f};
    bool sequential = false;      // --sequential: a --batch as one estimate after the other (default: rtdd_estimate_depth_batch, all images in the same launches)
    bool cold = false;            // --cold: no warm-up: the first (and, without --live, only) estimate pays the one-time costs
    // --regions cut|smooth|both, --region-fill, --region-wand: rtdd_region_flags and what is painted into the pyramid's region pair
    int region_flags = 0;
    std::vector<Lasso> region_fills;
    std::vector<Wand> region_wands;
    // --region-surface "x,y,step[,below,above]:id" (after --surface-global: every pixel in the band): rtdd_fill_surface after the estimate
    std::vector<rtdd_surface_wand> region_surfaces;
    // --segment "step[,lo,hi[,minPixels[,maxRegions[,firstCode]]]]": rtdd_segment_surfaces after the estimate, behind the clicks above
    bool segment = false;
    rtdd_segmentation segmentation{};
    bool edges_color = false;     // --edges color: the estimates read their edge weights from the BGR image (rtdd_pyramid_set_guide); default gray: the reference's
    // --layer sprite --layer-alpha alpha --layer-at x,y [--layer-scale S] [--layer-filter nearest|bilinear] [--layer-depth z | --layer-plane
    // x0,y0,z0,x1,y1,z1] [--layer-feather f] [--layer-opacity o]: rtdd_composite_layer after the estimate; --effect then runs on the composite
    // and ITS depth map.  sprite: B, G, R, A interleaved, rows and cols in `layer`
    bool has_layer = false;
    std::vector<unsigned char> sprite;
    rtdd_layer layer = {0, 0, 0, 0, 256, RTDD_LAYER_NEAREST, 255, 0, 0, 0, 0, 128.0f, 128.0f, 0.0f};
    // --remove-region ID [--remove-grow N] [--remove-behind D]: rtdd_remove_object after the estimate, the region's code plane the mask;
    // --move-region ID:dx,dy[:depth]: rtdd_lift_layer, rtdd_remove_object and rtdd_composite_layer of the sprite (dx, dy) away, at `depth`
    // or at the region's own nearest depth.  Before --layer and --effect, which run on the result and ITS depth map
    bool has_remove = false, has_move = false, move_has_depth = false;
    rtdd_removal removal = {0, 0, 0.0f};                            // select: the region id
    int move_dx = 0, move_dy = 0;
    float move_depth = 0.0f;
    // --effect parallax --plate-region ID [--remove-grow N] [--remove-behind D]: the painted region removed (rtdd_remove_object, `removal`)
    // into a background plate held aside -- the scene itself stays -- and the view rendered over both layers
    // (rtdd_simulate_parallax_layered); --parallax-depth-out FILE / --parallax-coverage FILE: its depth map (u8, as DepthMap) and coverage
    bool has_plate = false;
    std::string parallax_depth_out, parallax_coverage;
    // --select-grow R2 / --select-shrink R2: the region's code plane refined (rtdd_refine_mask) into the 0 / 255 mask the removal, the lift
    // and the plate read with select 0; --move-feather W: the lift's alpha is that mask feathered W pixels inwards (rtdd_lift_layer_matte)
    int select_op = -1, select_r2 = 0;                              // RTDD_REFINE_GROW or RTDD_REFINE_SHRINK; -1: the code plane as it is
    float move_feather = 0.0f;                                      // 0: a hard lift
};
// The mask --remove-region / --move-region / --plate-region read: the region's code plane under the region id, or (--select-grow /
// --select-shrink) that plane refined into `refined` (device, cols bytes a row), read under select 0.
static int region_mask(rtdd_ctx *ctx, const Job &job, unsigned char *refined, int rows, int cols, const uint8_t **mask, size_t *pitch, rtdd_removal *removal) {
    void *p_code; size_t pi_code;
    int rc = rtdd_pyramid_image(ctx, RTDD_IMG_REGION_CODE, 0, &p_code, &pi_code, nullptr, nullptr);
    if (rc != RTDD_OK) return rc;
    *mask = (const uint8_t *)p_code; *pitch = pi_code; *removal = job.removal;
    if (job.select_op < 0) return RTDD_OK;
    const rtdd_mask_refine r = {job.removal.select, job.select_op, job.select_r2, job.select_r2, 0.0f, 0.0f};
    rc = rtdd_refine_mask(ctx, (const uint8_t *)p_code, pi_code, rows, cols, &r, refined, (size_t)cols);
    *mask = refined; *pitch = (size_t)cols; removal->select = 0;
    return rc;
}
// what --parallax-depth-out and --parallax-coverage write: device 0's last view
struct ParallaxFiles { std::vector<unsigned char> depth_u8, coverage; };

// --stroke / --erase / --ramp: the job's strokes on a device image pair, one call
static int stroke_calls(rtdd_ctx *ctx, const Job &job, void *ed, size_t ed_pitch, void *scr, size_t scr_pitch, const void *orig, size_t orig_pitch, int rows, int cols) {
    if (job.strokes.empty()) return RTDD_OK;
    if (job.has_ramp) {
        CK(rtdd_paint_ramp_strokes(ctx, job.strokes.data(), (int)job.strokes.size(), (uint8_t *)ed, ed_pitch, (uint8_t *)scr, scr_pitch, (const uint8_t *)orig, orig_pitch, rows, cols));
        return RTDD_OK;
    }
    std::vector<rtdd_stroke> plain;
    for (const rtdd_ramp_stroke &q : job.strokes) plain.push_back(rtdd_stroke{q.x0, q.y0, q.x1, q.y1, q.radius, q.brush, q.label0});
    CK(rtdd_paint_strokes(ctx, plain.data(), (int)plain.size(), (uint8_t *)ed, ed_pitch, (uint8_t *)scr, scr_pitch, (const uint8_t *)orig, orig_pitch, rows, cols));
    return RTDD_OK;
}

// --fill / --fill-erase: the job's polygons on a device image pair, one call each
static int fill_polygons(rtdd_ctx *ctx, const Job &job, void *ed, size_t ed_pitch, void *scr, size_t scr_pitch, const void *orig, size_t orig_pitch, int rows, int cols) {
    for (const Job::Lasso &l : job.fills)
        CK(rtdd_fill_polygon(ctx, l.xy.data(), (int)l.xy.size() / 2, &l.fill, (uint8_t *)ed, ed_pitch, (uint8_t *)scr, scr_pitch, (const uint8_t *)orig, orig_pitch, rows, cols));
    return RTDD_OK;
}

// "x,y;x,y;..." and, when the polygon paints, ":label" or ":label0,label1,ax0,ay0,ax1,ay1"
static bool parse_fill(const char *arg, bool erase, int rule, Job::Lasso *l) {
    l->xy.clear();
    l->fill = rtdd_fill{rule, 0, 0, 0, 0, RTDD_STROKE_ERASE, RTDD_STROKE_ERASE};
    for (;;) {
        int x, y, n = 0;
        if (std::sscanf(arg, "%d,%d%n", &x, &y, &n) != 2 || n == 0) return false;
        l->xy.push_back(x); l->xy.push_back(y);
        arg += n;
        if (*arg != ';') break;
        arg++;
    }
    if (erase) return *arg == 0;
    if (*arg != ':') return false;
    int n = 0;
    rtdd_fill &f = l->fill;
    if (std::sscanf(arg + 1, "%d,%d,%d,%d,%d,%d%n", &f.label0, &f.label1, &f.ax0, &f.ay0, &f.ax1, &f.ay1, &n) == 6 && arg[1 + n] == 0) return true;
    f = rtdd_fill{rule, 0, 0, 0, 0, 0, 0};
    n = 0;
    if (std::sscanf(arg + 1, "%d%n", &f.label0, &n) != 1 || arg[1 + n] != 0) return false;
    f.label1 = f.label0;
    return true;
}

// --wand / --wand-erase: the job's clicks on a device image pair, one call each (each synchronises); prints what each covered
static int wand_calls(rtdd_ctx *ctx, const Job &job, void *ed, size_t ed_pitch, void *scr, size_t scr_pitch, const void *orig, size_t orig_pitch, int rows, int cols) {
    for (const Job::Wand &q : job.wands) {
        rtdd_wand_info info;
        CK(rtdd_fill_similar(ctx, &q.w, (uint8_t *)ed, ed_pitch, (uint8_t *)scr, scr_pitch, (const uint8_t *)orig, orig_pitch, rows, cols, &info));
        std::printf("wand %d,%d tolerance %d: %d pixels, x %d..%d, y %d..%d\n", q.w.x, q.w.y, q.w.tolerance, info.pixels, info.x0, info.x1, info.y0, info.y1);
    }
    return RTDD_OK;
}

// "x,y,tol" and, when the wand paints, ":label" or ":label0,label1,ax0,ay0,ax1,ay1"; with "F:" in front when `frame` is asked for
static bool parse_wand(const char *arg, bool erase, int flags, rtdd_wand *w, int *frame) {
    int n = 0;
    if (frame) { if (std::sscanf(arg, "%d:%n", frame, &n) != 1 || n == 0) return false; arg += n; n = 0; }
    *w = rtdd_wand{0, 0, 0, flags, 0, 0, 0, 0, RTDD_STROKE_ERASE, RTDD_STROKE_ERASE};
    if (std::sscanf(arg, "%d,%d,%d%n", &w->x, &w->y, &w->tolerance, &n) != 3 || n == 0) return false;
    arg += n;
    if (erase) return *arg == 0;
    if (*arg != ':') return false;
    n = 0;
    if (std::sscanf(arg + 1, "%d,%d,%d,%d,%d,%d%n", &w->label0, &w->label1, &w->ax0, &w->ay0, &w->ax1, &w->ay1, &n) == 6 && arg[1 + n] == 0) return true;
    w->ax0 = w->ay0 = w->ax1 = w->ay1 = 0;
    n = 0;
    if (std::sscanf(arg + 1, "%d%n", &w->label0, &n) != 1 || arg[1 + n] != 0) return false;
    w->label1 = w->label0;
    return true;
}

// --stroke / --erase / --ramp: the job's strokes on a device image pair, one call; the --fill / --fill-erase polygons behind them, the
// --wand / --wand-erase clicks behind those
static int paint_strokes(rtdd_ctx *ctx, const Job &job, void *ed, size_t ed_pitch, void *scr, size_t scr_pitch, const void *orig, size_t orig_pitch, int rows, int cols) {
    CK(stroke_calls(ctx, job, ed, ed_pitch, scr, scr_pitch, orig, orig_pitch, rows, cols));
    CK(fill_polygons(ctx, job, ed, ed_pitch, scr, scr_pitch, orig, orig_pitch, rows, cols));
    return wand_calls(ctx, job, ed, ed_pitch, scr, scr_pitch, orig, orig_pitch, rows, cols);
}

// --regions: the flags, then the --region-fill polygons and the --region-wand clicks on the selected image's region pair (the label is the
// region id; "similar" reads the photograph).  Behind rtdd_pyramid_set_image, which makes the image's regions unassigned again
static int region_calls(rtdd_ctx *ctx, const Job &job, const void *orig, size_t orig_pitch, int rows, int cols) {
    if (job.region_flags == 0) return RTDD_OK;
    CK(rtdd_pyramid_set_regions(ctx, job.region_flags));
    void *pe, *pm; size_t pie, pim;
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_REGION_EDITED, 0, &pe, &pie, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_REGION_MASK, 0, &pm, &pim, nullptr, nullptr));
    for (const Job::Lasso &l : job.region_fills)
        CK(rtdd_fill_polygon(ctx, l.xy.data(), (int)l.xy.size() / 2, &l.fill, (uint8_t *)pe, pie, (uint8_t *)pm, pim, (const uint8_t *)orig, orig_pitch, rows, cols));
    for (const Job::Wand &q : job.region_wands) {
        rtdd_wand_info info;
        CK(rtdd_fill_similar(ctx, &q.w, (uint8_t *)pe, pie, (uint8_t *)pm, pim, (const uint8_t *)orig, orig_pitch, rows, cols, &info));
        std::printf("region wand %d,%d tolerance %d: region %d, %d pixels\n", q.w.x, q.w.y, q.w.tolerance, q.w.label0, info.pixels);
    }
    return RTDD_OK;
}

// --region-surface: the clicks on the estimate's own depth map (level 0) into the region pair, one rtdd_fill_surface call each (each
// synchronises); then the level-0 code plane, which --remove-region / --move-region / --plate-region read, is filled again from the pair
static int region_surface_calls(rtdd_ctx *ctx, const Job &job, const void *depth, size_t depth_pitch, int rows, int cols) {
    if (job.region_surfaces.empty() && !job.segment) return RTDD_OK;
    void *pe, *pm, *pc; size_t pie, pim, pic;
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_REGION_EDITED, 0, &pe, &pie, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_REGION_MASK, 0, &pm, &pim, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_REGION_CODE, 0, &pc, &pic, nullptr, nullptr));
    for (const rtdd_surface_wand &w : job.region_surfaces) {
        rtdd_wand_info info;
        CK(rtdd_fill_surface(ctx, &w, (uint8_t *)pe, pie, (uint8_t *)pm, pim, nullptr, 0, (const float *)depth, depth_pitch, rows, cols, &info));
        std::printf("region surface %d,%d step %g band %g,%g%s: region %d, %d pixels, x %d..%d, y %d..%d\n", w.x, w.y, w.step, w.below, w.above,
                    (w.flags & RTDD_SURFACE_GLOBAL) ? " global" : "", w.label0, info.pixels, info.x0, info.x1, info.y0, info.y1);
    }
    if (job.segment) {                                                // --segment: every surface at once, one line per region
        std::vector<rtdd_segment> seg((size_t)job.segmentation.maxRegions);
        rtdd_segment_info info;
        CK(rtdd_segment_surfaces(ctx, &job.segmentation, (uint8_t *)pe, pie, (uint8_t *)pm, pim, (const float *)depth, depth_pitch, nullptr, 0, rows, cols,
                                 seg.data(), &info));
        std::printf("segment step %g band %g,%g minPixels %d: %d components, %d candidates, %d regions, %d pixels\n", job.segmentation.step, job.segmentation.lo,
                    job.segmentation.hi, job.segmentation.minPixels, info.components, info.candidates, info.regions, info.pixels);
        for (int k = 0; k < info.regions; k++)
            std::printf("segment region %d: %d pixels, root %d,%d, x %d..%d, y %d..%d, depth %.9g..%.9g\n", seg[k].code, seg[k].pixels, seg[k].rootX, seg[k].rootY,
                        seg[k].x0, seg[k].x1, seg[k].y0, seg[k].y1, seg[k].dmin, seg[k].dmax);
    }
    return rtdd_region_codes(ctx, (const uint8_t *)pe, pie, (const uint8_t *)pm, pim, rows, cols, 0, (uint8_t *)pc, pic);
}

// "step", "step,lo,hi", "step,lo,hi,minPixels", "...,maxRegions", "...,firstCode" (the library checks the values)
static bool parse_segment(const char *arg, rtdd_segmentation *g) {
    *g = rtdd_segmentation{0.0f, 0.0f, 255.0f, 64, 8, 1, 0};
    int n = 0;
    const int got = std::sscanf(arg, "%f%n,%f,%f%n,%d%n,%d%n,%d%n", &g->step, &n, &g->lo, &g->hi, &n, &g->minPixels, &n, &g->maxRegions, &n, &g->firstCode, &n);
    return got >= 1 && got != 2 && n > 0 && arg[n] == 0;
}

// "x,y,step:id" or "x,y,step,below,above:id"
static bool parse_surface(const char *arg, int flags, rtdd_surface_wand *w) {
    *w = rtdd_surface_wand{0, 0, 0.0f, 255.0f, 255.0f, flags, 0, 0, 0, 0, 0, 0};
    int n = 0;
    if (std::sscanf(arg, "%d,%d,%f,%f,%f:%d%n", &w->x, &w->y, &w->step, &w->below, &w->above, &w->label0, &n) == 6 && n > 0 && arg[n] == 0) { w->label1 = w->label0; return true; }
    w->below = w->above = 255.0f; n = 0;
    if (std::sscanf(arg, "%d,%d,%f:%d%n", &w->x, &w->y, &w->step, &w->label0, &n) == 4 && n > 0 && arg[n] == 0) { w->label1 = w->label0; return true; }
    return false;
}

// rtdd_paint_ramp_strokes (with label0 == label1: rtdd_paint_strokes) restated for the host's own image pair (--live: the host owns the pair every frame uploads; include/rtdd.h has the
// rules).  Dense images; `orig` is the BGR image.  Returns whether a stroke erased.
static bool host_strokes(const std::vector<rtdd_ramp_stroke> &strokes, unsigned char *scr, unsigned char *ed, const unsigned char *orig, int rows, int cols) {
    typedef long long i64; typedef unsigned long long u64;
    bool erased = false;
    for (const rtdd_ramp_stroke &q : strokes) {
        const int h = q.radius / 2;
        const int xa = std::max(std::min(q.x0, q.x1) - h, 0), xb = std::min(std::max(q.x0, q.x1) + h, cols - 1);
        const int ya = std::max(std::min(q.y0, q.y1) - h, 0), yb = std::min(std::max(q.y0, q.y1) + h, rows - 1);
        const i64 dx = q.x1 - q.x0, dy = q.y1 - q.y0, dd = dx * dx + dy * dy, r2 = (i64)q.radius * q.radius;
        erased = erased || q.label0 == RTDD_STROKE_ERASE;
        for (int y = ya; y <= yb; y++)
            for (int x = xa; x <= xb; x++) {
                const i64 vx = x - q.x0, vy = y - q.y0, cross = dx * vy - dy * vx, t = vx * dx + vy * dy;
                const u64 ac = (u64)(cross < 0 ? -cross : cross);
                bool in;
                if (q.brush == RTDD_BRUSH_SQUARE) in = ac <= (u64)h * (u64)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
                else if (t <= 0) in = 4 * (vx * vx + vy * vy) <= r2;
                else if (t >= dd) in = 4 * ((i64)(x - q.x1) * (x - q.x1) + (i64)(y - q.y1) * (y - q.y1)) <= r2;
                else in = 2 * ac < (1ull << 32) && (2 * ac) * (2 * ac) <= (u64)r2 * (u64)dd;      // (beyond 2^32 the square exceeds radius^2 |d|^2 <= 2^54)
                if (!in) continue;
                const size_t i = (size_t)y * cols + x;
                if (q.label0 == RTDD_STROKE_ERASE) { scr[i] = 0; for (int c = 0; c < 3; c++) ed[3 * i + c] = orig[3 * i + c]; continue; }
                i64 label = q.label0;                                   // the ramp: the label at the foot of the perpendicular, rounded half up
                if (dd != 0) { const i64 tc = std::min(std::max(t, (i64)0), dd); label = (2 * (q.label0 * (dd - tc) + q.label1 * tc) + dd) / (2 * dd); }
                scr[i] = 255; for (int c = 0; c < 3; c++) ed[3 * i + c] = (unsigned char)label;
            }
    }
    return erased;
}

// rtdd_fill_similar restated for the host's own image pair (--live, like host_strokes; include/rtdd.h has the rule): the component by a
// queue.  Dense images; `orig` is the BGR image; the wand is valid (checked by its caller).  Returns the number of covered pixels.
static int host_wand(const rtdd_wand &w, unsigned char *scr, unsigned char *ed, const unsigned char *orig, int rows, int cols) {
    typedef long long i64;
    const size_t npx = (size_t)rows * cols, seed = (size_t)w.y * cols + w.x;
    auto similar = [&](size_t i) {
        for (int c = 0; c < 3; c++) if (std::abs((int)orig[3 * i + c] - (int)orig[3 * seed + c]) > w.tolerance) return false;
        return true;
    };
    std::vector<unsigned char> in(npx, 0);
    if (w.flags & RTDD_WAND_GLOBAL) { for (size_t i = 0; i < npx; i++) in[i] = similar(i); }
    else {
        std::vector<size_t> todo(1, seed);
        in[seed] = 1;
        while (!todo.empty()) {
            const size_t i = todo.back(); todo.pop_back();
            const int x = (int)(i % cols), y = (int)(i / cols);
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if ((dx == 0 && dy == 0) || (dx != 0 && dy != 0 && !(w.flags & RTDD_WAND_CONNECT_8))) continue;
                    const int qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= cols || qy < 0 || qy >= rows) continue;
                    const size_t j = (size_t)qy * cols + qx;
                    if (!in[j] && similar(j)) { in[j] = 1; todo.push_back(j); }
                }
        }
    }
    const i64 dx = w.ax1 - w.ax0, dy = w.ay1 - w.ay0, dd = dx * dx + dy * dy;
    int covered = 0;
    for (size_t i = 0; i < npx; i++) {
        if (!in[i]) continue;
        covered++;
        if (w.label0 == RTDD_STROKE_ERASE) { scr[i] = 0; for (int c = 0; c < 3; c++) ed[3 * i + c] = orig[3 * i + c]; continue; }
        i64 label = w.label0;
        if (dd != 0 && w.label0 != w.label1) {
            const i64 t = std::min(std::max(((i64)(i % cols) - w.ax0) * dx + ((i64)(i / cols) - w.ay0) * dy, (i64)0), dd);
            label = (2 * (w.label0 * (dd - t) + w.label1 * t) + dd) / (2 * dd);
        }
        scr[i] = 255; for (int c = 0; c < 3; c++) ed[3 * i + c] = (unsigned char)label;
    }
    return covered;
}

// "x0,y0,x1,y1,label,radius[,round]" (kind 'e', erase: no label; kind 'r', ramp: label0,label1), with "F:" in front when `frame` is asked for
static bool parse_stroke(const char *arg, char kind, rtdd_ramp_stroke *q, int *frame) {
    int n = 0;
    if (frame) { if (std::sscanf(arg, "%d:%n", frame, &n) != 1 || n == 0) return false; arg += n; n = 0; }
    q->label0 = RTDD_STROKE_ERASE; q->brush = RTDD_BRUSH_SQUARE;
    if (kind == 'e' ? std::sscanf(arg, "%d,%d,%d,%d,%d%n", &q->x0, &q->y0, &q->x1, &q->y1, &q->radius, &n) != 5
        : kind == 'r' ? std::sscanf(arg, "%d,%d,%d,%d,%d,%d,%d%n", &q->x0, &q->y0, &q->x1, &q->y1, &q->label0, &q->label1, &q->radius, &n) != 7
                      : std::sscanf(arg, "%d,%d,%d,%d,%d,%d%n", &q->x0, &q->y0, &q->x1, &q->y1, &q->label0, &q->radius, &n) != 6) return false;
    if (kind != 'r') q->label1 = q->label0;
    if (!std::strcmp(arg + n, ",round")) q->brush = RTDD_BRUSH_ROUND;
    else if (arg[n] != 0 && std::strcmp(arg + n, ",square")) return false;
    return true;
}

// What a process pays ONCE on a device -- the runtime's first stream and allocations, every kernel's code object on its first launch,
// ~20 ms together -- and what "Processing Time" is not about (the reference's first key press pays CUDA's likewise): a 96 x 128 estimate
// and each effect on a context of its own, destroyed again.  Nothing of the job's is touched; --cold leaves it out.
static void warm_up(int device) {
    rtdd_ctx *w = nullptr;
    if (rtdd_ctx_create(device, &w) != RTDD_OK) return;
    const int rows = 96, cols = 128;
    std::vector<unsigned char> bgr((size_t)rows * cols * 3, 90), ann((size_t)rows * cols, 32);
    for (int x = 20; x < 40; x++) { ann[(size_t)30 * cols + x] = 254; ann[(size_t)70 * cols + x] = 0; }
    unsigned char *d_bgr = nullptr, *d_ann = nullptr;
    if (hipSetDevice(device) == hipSuccess && hipMalloc((void **)&d_bgr, bgr.size()) == hipSuccess && hipMalloc((void **)&d_ann, ann.size()) == hipSuccess &&
        rtdd_load_weights(w, 0.4f) == RTDD_OK && rtdd_pyramid_create(w, rows, cols) == RTDD_OK &&
        rtdd_upload(w, d_bgr, (size_t)cols * 3, bgr.data(), (size_t)cols * 3, (size_t)cols * 3, rows) == RTDD_OK && rtdd_pyramid_set_image(w, d_bgr, (size_t)cols * 3) == RTDD_OK &&
        rtdd_upload(w, d_ann, cols, ann.data(), cols, cols, rows) == RTDD_OK && rtdd_pyramid_set_annotation(w, d_ann, cols) == RTDD_OK && rtdd_estimate_depth(w, 1000) == RTDD_OK) {
        void *po, *pg, *pd, *pa; size_t io, ig, id, ia;
        if (rtdd_pyramid_image(w, RTDD_IMG_ORIGINAL, 0, &po, &io, nullptr, nullptr) == RTDD_OK && rtdd_pyramid_image(w, RTDD_IMG_GRAY, 0, &pg, &ig, nullptr, nullptr) == RTDD_OK &&
            rtdd_pyramid_image(w, RTDD_IMG_DEPTH, 0, &pd, &id, nullptr, nullptr) == RTDD_OK && rtdd_pyramid_image(w, RTDD_IMG_ARTISTIC, 0, &pa, &ia, nullptr, nullptr) == RTDD_OK) {
            (void)rtdd_simulate_defocus(w, (const uint8_t *)po, io, (const float *)pd, id, (uint8_t *)pa, ia, rows, cols);
            (void)rtdd_simulate_desaturation(w, (const uint8_t *)po, io, (const uint8_t *)pg, ig, (const float *)pd, id, (uint8_t *)pa, ia, rows, cols);
            (void)rtdd_simulate_haze(w, (const uint8_t *)po, io, (const float *)pd, id, (uint8_t *)pa, ia, rows, cols);
        }
        std::vector<unsigned char> back((size_t)rows * cols);
        void *pu; size_t iu;
        if (rtdd_pyramid_image(w, RTDD_IMG_DEPTH_U8, 0, &pu, &iu, nullptr, nullptr) == RTDD_OK) (void)rtdd_download(w, back.data(), cols, pu, iu, cols, rows);
    }
    (void)rtdd_ctx_synchronize(w);
    if (d_bgr) (void)hipFree(d_bgr);
    if (d_ann) (void)hipFree(d_ann);
    (void)rtdd_ctx_destroy(w);
}

// One GPU: context + stream + device staging, runs `count` estimates; keeps the last result on the host.
static int run_device(int device, const Job &job, int count, bool live, std::vector<unsigned char> *depth_u8, std::vector<unsigned char> *art, double *ms_per_estimate,
                      std::vector<std::vector<unsigned char>> *every_map = nullptr, std::vector<unsigned char> *annotated = nullptr,
                      ParallaxFiles *parallax_files = nullptr) {
    // everything this function owns, released on EVERY return path (the CK() early returns included)
    struct Owned {
        rtdd_ctx *ctx = nullptr; hipStream_t stream = nullptr; unsigned char *d_bgr = nullptr, *d_ann = nullptr;
        unsigned char *d_sprite = nullptr, *d_lart = nullptr; float *d_lz = nullptr;      // --layer: the sprite, the composite and its depth map
        unsigned char *d_rart = nullptr, *d_msprite = nullptr, *d_mart = nullptr; float *d_rz = nullptr, *d_mz = nullptr;     // --remove-region / --move-region
        unsigned char *d_part = nullptr, *d_pz8 = nullptr, *d_pcov = nullptr; float *d_pplz = nullptr, *d_pz = nullptr;          // --plate-region: the plate; the view's depth map (f32, u8) and coverage
        unsigned char *d_sel = nullptr, *d_alpha = nullptr;                                  // --select-grow / --select-shrink: the refined mask; --move-feather: the lift's alpha
        ~Owned() {
            if (d_bgr) (void)hipFree(d_bgr);
            if (d_ann) (void)hipFree(d_ann);
            if (d_sprite) (void)hipFree(d_sprite);
            if (d_lart) (void)hipFree(d_lart);
            if (d_lz) (void)hipFree(d_lz);
            if (d_rart) (void)hipFree(d_rart);
            if (d_rz) (void)hipFree(d_rz);
            if (d_msprite) (void)hipFree(d_msprite);
            if (d_mart) (void)hipFree(d_mart);
            if (d_mz) (void)hipFree(d_mz);
            if (d_part) (void)hipFree(d_part);
            if (d_pplz) (void)hipFree(d_pplz);
            if (d_pz) (void)hipFree(d_pz);
            if (d_pz8) (void)hipFree(d_pz8);
            if (d_pcov) (void)hipFree(d_pcov);
            if (d_sel) (void)hipFree(d_sel);
            if (d_alpha) (void)hipFree(d_alpha);
            if (ctx) rtdd_ctx_destroy(ctx);           // synchronises the stream first
            if (stream) (void)hipStreamDestroy(stream);
        }
    } own;
    if (!job.cold) warm_up(device);
    int rc = rtdd_ctx_create(device, &own.ctx);
    if (rc != RTDD_OK) { std::printf("rtdd_ctx_create(%d): %s\n", device, rtdd_status_string(rc)); return rc; }
    rtdd_ctx *ctx = own.ctx;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&own.stream) != hipSuccess) { std::printf("device %d: cannot create a stream\n", device); return RTDD_ERR_HIP; }
    rtdd_ctx_set_stream(ctx, own.stream);
    const int rows = job.bgr.h, cols = job.bgr.w;
    CK(rtdd_load_weights(ctx, 0.4f));                                   // main.cpp:152-155
    // --batch B without an effect or a refinement: this device's images as ONE batched pyramid -- every level of all of them in the same
    // launches (rtdd_estimate_depth_batch: the coarse levels of one 1080p image use a quarter of the chip)
    const bool batched = !live && count > 1 && !job.sequential && job.effect.empty() && job.refine.empty() && !job.has_layer && !job.has_remove && !job.has_move;
    if (batched) {
        CK(rtdd_pyramid_create_batch(ctx, rows, cols, count));
        if (job.edges_color) CK(rtdd_pyramid_set_guide(ctx, RTDD_GUIDE_BGR));
        if (hipMalloc((void **)&own.d_bgr, (size_t)rows * cols * 3) != hipSuccess || hipMalloc((void **)&own.d_ann, (size_t)rows * cols) != hipSuccess) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
        auto t0 = std::chrono::steady_clock::now();
        for (int n = 0; n < count; n++) {                               // every image is independent: its own upload, annotation and strokes
            void *ps, *pe; size_t pis, pie;
            CK(rtdd_pyramid_select(ctx, n));
            CK(rtdd_upload(ctx, own.d_bgr, (size_t)cols * 3, job.bgr.px.data(), (size_t)cols * 3, (size_t)cols * 3, rows));
            CK(rtdd_pyramid_set_image(ctx, own.d_bgr, (size_t)cols * 3));
            if (job.has_ann) {
                CK(rtdd_upload(ctx, own.d_ann, cols, job.ann.px.data(), cols, cols, rows));
                CK(rtdd_pyramid_set_annotation(ctx, own.d_ann, cols));
            }
            CK(rtdd_pyramid_image(ctx, RTDD_IMG_SCRIBBLE, 0, &ps, &pis, nullptr, nullptr));
            CK(rtdd_pyramid_image(ctx, RTDD_IMG_EDITED, 0, &pe, &pie, nullptr, nullptr));
            for (const Paint &p : job.paints) CK(rtdd_paint_image(ctx, p.x, p.y, p.label, p.radius, (uint8_t *)pe, pie, (uint8_t *)ps, pis, rows, cols));
            void *po; size_t pio;
            CK(rtdd_pyramid_image(ctx, RTDD_IMG_ORIGINAL, 0, &po, &pio, nullptr, nullptr));
            CK(paint_strokes(ctx, job, pe, pie, ps, pis, po, pio, rows, cols));
            CK(region_calls(ctx, job, po, pio, rows, cols));
        }
        CK(rtdd_estimate_depth_batch(ctx, job.iters));                  // main.cpp:239-291, for every image
        depth_u8->resize((size_t)rows * cols);
        for (int n = 0; n < count; n++) {
            void *pu; size_t piu;
            CK(rtdd_pyramid_select(ctx, n));
            CK(rtdd_pyramid_image(ctx, RTDD_IMG_DEPTH_U8, 0, &pu, &piu, nullptr, nullptr));
            CK(rtdd_download(ctx, depth_u8->data(), cols, pu, piu, cols, rows));      // main.cpp:291 (synchronises)
            if (every_map) every_map->push_back(*depth_u8);
        }
        *ms_per_estimate = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / count;
        if (annotated) {
            void *pe; size_t pie;
            CK(rtdd_pyramid_select(ctx, 0));
            CK(rtdd_pyramid_image(ctx, RTDD_IMG_EDITED, 0, &pe, &pie, nullptr, nullptr));
            annotated->resize((size_t)rows * cols * 3); CK(rtdd_download(ctx, annotated->data(), (size_t)cols * 3, pe, pie, (size_t)cols * 3, rows));
        }
        CK(rtdd_ctx_synchronize(ctx));
        return RTDD_OK;
    }
    CK(rtdd_pyramid_create(ctx, rows, cols));                           // main.cpp:92-149
    if (job.edges_color) CK(rtdd_pyramid_set_guide(ctx, RTDD_GUIDE_BGR));  // (single estimates, --live and --sequential alike)
    if (hipMalloc((void **)&own.d_bgr, (size_t)rows * cols * 3) != hipSuccess || hipMalloc((void **)&own.d_ann, (size_t)rows * cols) != hipSuccess) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
    unsigned char *d_bgr = own.d_bgr, *d_ann = own.d_ann;
    void *p_scr, *p_ed, *p_orig, *p_gray, *p_depth, *p_art, *p_u8;
    size_t pi_scr, pi_ed, pi_orig, pi_gray, pi_depth, pi_art, pi_u8;
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_SCRIBBLE, 0, &p_scr, &pi_scr, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_EDITED, 0, &p_ed, &pi_ed, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_ORIGINAL, 0, &p_orig, &pi_orig, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_GRAY, 0, &p_gray, &pi_gray, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_DEPTH, 0, &p_depth, &pi_depth, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_ARTISTIC, 0, &p_art, &pi_art, nullptr, nullptr));
    CK(rtdd_pyramid_image(ctx, RTDD_IMG_DEPTH_U8, 0, &p_u8, &pi_u8, nullptr, nullptr));
    if (job.has_layer) {                                                // --layer: the sprite goes up once; the composite and its depth map get images of their own
        const size_t sw = (size_t)job.layer.cols * 4;
        if (hipMalloc((void **)&own.d_sprite, sw * job.layer.rows) != hipSuccess || hipMalloc((void **)&own.d_lart, (size_t)rows * cols * 3) != hipSuccess ||
            hipMalloc((void **)&own.d_lz, (size_t)rows * cols * 4) != hipSuccess) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
        CK(rtdd_upload(ctx, own.d_sprite, sw, job.sprite.data(), sw, sw, job.layer.rows));
    }
    if (job.has_remove || job.has_move) {                               // --remove-region / --move-region: the scene without the object, and where it is moved its sprite and the scene with it again
        const size_t px = (size_t)rows * cols;
        bool ok = hipMalloc((void **)&own.d_rart, px * 3) == hipSuccess && hipMalloc((void **)&own.d_rz, px * 4) == hipSuccess;
        if (ok && job.has_move) ok = hipMalloc((void **)&own.d_msprite, px * 4) == hipSuccess && hipMalloc((void **)&own.d_mart, px * 3) == hipSuccess && hipMalloc((void **)&own.d_mz, px * 4) == hipSuccess;
        if (!ok) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
    }
    if (job.select_op >= 0 && hipMalloc((void **)&own.d_sel, (size_t)rows * cols) != hipSuccess) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
    if (job.move_feather > 0.0f && hipMalloc((void **)&own.d_alpha, (size_t)rows * cols) != hipSuccess) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
    const bool want_pz = !job.parallax_depth_out.empty(), want_pcov = !job.parallax_coverage.empty();
    if (job.has_plate || want_pz || want_pcov) {                       // --plate-region, --parallax-depth-out, --parallax-coverage
        const size_t px = (size_t)rows * cols;
        bool ok = true;
        if (job.has_plate) ok = hipMalloc((void **)&own.d_part, px * 3) == hipSuccess && hipMalloc((void **)&own.d_pplz, px * 4) == hipSuccess;
        if (ok && want_pz) ok = hipMalloc((void **)&own.d_pz, px * 4) == hipSuccess && hipMalloc((void **)&own.d_pz8, px) == hipSuccess;
        if (ok && want_pcov) ok = hipMalloc((void **)&own.d_pcov, px) == hipSuccess;
        if (!ok) { std::printf("device %d: out of memory\n", device); return RTDD_ERR_NOMEM; }
    }

    // --live N: the reference's frame loop as it clocks it (main.cpp:232-295) -- every frame uploads the host's scribble and edited
    // images (:236-237), estimates, downloads the u8 map (:290-291) -- two frames in flight (rtdd_live_submit_ex): the copies of one frame
    // overlap the arithmetic of the other.  With --effect X every frame also renders the sticky effect from its own depth map and brings
    // the artistic image to the host (main.cpp:190-230 runs in every iteration of the loop once a key has switched the effect on).
    if (live && job.refine.empty()) {
        struct Pinned { void *p = nullptr; ~Pinned() { if (p) rtdd_host_free(p); } } h_scr, h_ed, h_u8[2], h_art[2];
        const int fx = job.effect == "defocus" ? RTDD_EFFECT_DEFOCUS : job.effect == "desaturation" ? RTDD_EFFECT_DESATURATION : job.effect == "haze" ? RTDD_EFFECT_HAZE : RTDD_EFFECT_NONE;
        if (fx != RTDD_EFFECT_NONE) { CK(rtdd_host_alloc(&h_art[0].p, (size_t)rows * cols * 3)); CK(rtdd_host_alloc(&h_art[1].p, (size_t)rows * cols * 3)); art->resize((size_t)rows * cols * 3); }
        CK(rtdd_upload(ctx, d_bgr, (size_t)cols * 3, job.bgr.px.data(), (size_t)cols * 3, (size_t)cols * 3, rows));
        CK(rtdd_pyramid_set_image(ctx, d_bgr, (size_t)cols * 3));
        if (job.has_ann) {
            CK(rtdd_upload(ctx, d_ann, cols, job.ann.px.data(), cols, cols, rows));
            CK(rtdd_pyramid_set_annotation(ctx, d_ann, cols));
        }
        for (const Paint &p : job.paints)
            CK(rtdd_paint_image(ctx, p.x, p.y, p.label, p.radius, (uint8_t *)p_ed, pi_ed, (uint8_t *)p_scr, pi_scr, rows, cols));
        CK(paint_strokes(ctx, job, p_ed, pi_ed, p_scr, pi_scr, p_orig, pi_orig, rows, cols));
        CK(region_calls(ctx, job, p_orig, pi_orig, rows, cols));
        CK(rtdd_host_alloc(&h_scr.p, (size_t)rows * cols)); CK(rtdd_host_alloc(&h_ed.p, (size_t)rows * cols * 3));
        CK(rtdd_host_alloc(&h_u8[0].p, (size_t)rows * cols)); CK(rtdd_host_alloc(&h_u8[1].p, (size_t)rows * cols));
        CK(rtdd_download(ctx, h_scr.p, cols, p_scr, pi_scr, cols, rows));            // the host's Mats (main.cpp:160-168: decoded on the host there)
        CK(rtdd_download(ctx, h_ed.p, (size_t)cols * 3, p_ed, pi_ed, (size_t)cols * 3, rows));
        depth_u8->resize((size_t)rows * cols);
        auto landed = [&](int f) {
            std::memcpy(depth_u8->data(), h_u8[f % 2].p, depth_u8->size());
            if (fx != RTDD_EFFECT_NONE) std::memcpy(art->data(), h_art[f % 2].p, art->size());
            if (every_map) every_map->push_back(*depth_u8);
        };
        auto t0 = std::chrono::steady_clock::now();
        for (int n = 0; n < count; n++) {
            bool painted = false;
            for (const Paint &p : job.live_paints)
                if (p.frame == n) {
                    // main.cpp:46-62: the mouse callback paints the DEVICE images and downloads them into the host's Mats, which the next
                    // estimate uploads again (:236-237).  The frames in flight are let land first: they read the images being painted.
                    if (!painted) {
                        while (rtdd_live_pending(ctx) > 0) { const int f = n - rtdd_live_pending(ctx); CK(rtdd_live_wait(ctx)); landed(f); }
                        // (an uploaded annotation pair becomes the pyramid's level-0 images: ask where they are now, include/rtdd.h)
                        CK(rtdd_pyramid_image(ctx, RTDD_IMG_SCRIBBLE, 0, &p_scr, &pi_scr, nullptr, nullptr));
                        CK(rtdd_pyramid_image(ctx, RTDD_IMG_EDITED, 0, &p_ed, &pi_ed, nullptr, nullptr));
                    }
                    CK(rtdd_paint_image(ctx, p.x, p.y, p.label, p.radius, (uint8_t *)p_ed, pi_ed, (uint8_t *)p_scr, pi_scr, rows, cols));
                    painted = true;
                }
            if (painted) {
                CK(rtdd_download(ctx, h_scr.p, cols, p_scr, pi_scr, cols, rows));
                CK(rtdd_download(ctx, h_ed.p, (size_t)cols * 3, p_ed, pi_ed, (size_t)cols * 3, rows));
            }
            // --stroke-at / --erase-at: the host owns the pair every frame uploads, so the strokes go onto the HOST images (the frames in
            // flight, which are still being uploaded from them, land first); after an erase the coarse levels are built afresh
            std::vector<rtdd_ramp_stroke> now;
            for (const LiveStroke &q : job.live_strokes) if (q.frame == n) now.push_back(q.s);
            if (!now.empty()) {
                while (rtdd_live_pending(ctx) > 0) { const int f = n - rtdd_live_pending(ctx); CK(rtdd_live_wait(ctx)); landed(f); }
                if (host_strokes(now, (unsigned char *)h_scr.p, (unsigned char *)h_ed.p, job.bgr.px.data(), rows, cols)) CK(rtdd_pyramid_annotation_rebuild(ctx));
            }
            // --wand-at / --wand-erase-at: likewise on the HOST images, behind the frame's strokes
            for (const Job::Wand &q : job.live_wands) {
                if (q.frame != n) continue;
                if (q.w.x < 0 || q.w.x >= cols || q.w.y < 0 || q.w.y >= rows || q.w.tolerance < 0 || q.w.tolerance > 255) { std::printf("--wand-at %d: the seed lies outside the image or the tolerance outside [0, 255]\n", n); return RTDD_ERR_INVALID; }
                while (rtdd_live_pending(ctx) > 0) { const int f = n - rtdd_live_pending(ctx); CK(rtdd_live_wait(ctx)); landed(f); }
                std::printf("frame %d: wand %d,%d tolerance %d: %d pixels\n", n, q.w.x, q.w.y, q.w.tolerance, host_wand(q.w, (unsigned char *)h_scr.p, (unsigned char *)h_ed.p, job.bgr.px.data(), rows, cols));
                if (q.w.label0 == RTDD_STROKE_ERASE) CK(rtdd_pyramid_annotation_rebuild(ctx));
            }
            if (rtdd_live_pending(ctx) >= 2) { const int f = n - 2; CK(rtdd_live_wait(ctx)); landed(f); }              // frame n-2's buffer is about to be reused
            CK(rtdd_live_submit_ex(ctx, (const uint8_t *)h_scr.p, cols, (const uint8_t *)h_ed.p, (size_t)cols * 3, job.iters, (uint8_t *)h_u8[n % 2].p, cols,
                                   fx, (uint8_t *)h_art[n % 2].p, (size_t)cols * 3));
        }
        while (rtdd_live_pending(ctx) > 0) { const int f = count - rtdd_live_pending(ctx); CK(rtdd_live_wait(ctx)); landed(f); }
        *ms_per_estimate = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (count > 0 ? count : 1);
        CK(rtdd_pyramid_image(ctx, RTDD_IMG_EDITED, 0, &p_ed, &pi_ed, nullptr, nullptr));
        if (annotated) { annotated->resize((size_t)rows * cols * 3); CK(rtdd_download(ctx, annotated->data(), (size_t)cols * 3, p_ed, pi_ed, (size_t)cols * 3, rows)); }
        CK(rtdd_ctx_synchronize(ctx));
        return RTDD_OK;
    }

    auto t0 = std::chrono::steady_clock::now();
    for (int n = 0; n < count; n++) {
        if (n == 0 || !live) {                                          // a new image (--batch: every image is independent -- rtdd_pyramid_set_image
                                                                        // also resets the warm-start state): upload + (re)build the pyramid inputs
            CK(rtdd_upload(ctx, d_bgr, (size_t)cols * 3, job.bgr.px.data(), (size_t)cols * 3, (size_t)cols * 3, rows));
            CK(rtdd_pyramid_set_image(ctx, d_bgr, (size_t)cols * 3));
            if (job.has_ann) {
                CK(rtdd_upload(ctx, d_ann, cols, job.ann.px.data(), cols, cols, rows));
                CK(rtdd_pyramid_set_annotation(ctx, d_ann, cols));
            }
            for (const Paint &p : job.paints)                           // main.cpp:55-57
                CK(rtdd_paint_image(ctx, p.x, p.y, p.label, p.radius, (uint8_t *)p_ed, pi_ed, (uint8_t *)p_scr, pi_scr, rows, cols));
            CK(paint_strokes(ctx, job, p_ed, pi_ed, p_scr, pi_scr, p_orig, pi_orig, rows, cols));
            CK(region_calls(ctx, job, p_orig, pi_orig, rows, cols));
        }
        CK(rtdd_estimate_depth(ctx, job.iters));                        // main.cpp:239-291
        if (!job.refine.empty()) {                                      // extension: converge the finest level
            rtdd_solve_params sp;
            sp.method = job.refine == "mg" ? RTDD_METHOD_MULTIGRID : job.refine == "auto" ? RTDD_METHOD_AUTO : RTDD_METHOD_RED_BLACK_GS;
            sp.maxIterations = job.refine == "mg" ? 100 : 400000; sp.tolerance = job.tolerance; sp.checkEvery = 0; sp.relaxation = RTDD_RELAXATION_AUTO;
            rtdd_solve_info si;
            CK(rtdd_refine_depth(ctx, &sp, &si));
            if (n == 0 && job.refine == "auto") std::printf("refine auto: %d cycles + %d sweeps, residual %g\n", si.cycles, si.iterations, si.residual);
            else if (n == 0) std::printf("refine %s: %d %s, residual %g\n", job.refine.c_str(), si.iterations, job.refine == "mg" ? "cycles" : "sweeps", si.residual);
        }
        // --region-surface, --segment: the regions clicked or found on the estimate's depth map, before anything below reads the level-0 code plane
        CK(region_surface_calls(ctx, job, p_depth, pi_depth, rows, cols));
        // --layer: the sprite is inserted after the estimate; the effect below then reads the composite and the composite's depth map
        // (desaturation's gray image stays the photograph's)
        // --remove-region / --move-region come first: the region's code plane (level 0, written by the estimate) is the mask, the id selects.
        // r_orig / r_depth: the scene without the object (--move-region: with it composited again where it went)
        void *r_orig = p_orig, *r_depth = p_depth;
        size_t ri_orig = pi_orig, ri_depth = pi_depth;
        if (job.has_remove || job.has_move) {
            const uint8_t *p_code; size_t pi_code; rtdd_removal removal;    // (--select-grow / --select-shrink: the refined mask, select 0)
            CK(region_mask(ctx, job, own.d_sel, rows, cols, &p_code, &pi_code, &removal));
            const size_t w3 = (size_t)cols * 3, w4 = (size_t)cols * 4;
            CK(rtdd_remove_object(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, p_code, pi_code, own.d_rart, w3, own.d_rz, w4, rows, cols, &removal));
            r_orig = own.d_rart; r_depth = own.d_rz; ri_orig = w3; ri_depth = w4;
            if (job.has_move) {
                // the sprite is the whole image's box, so it covers the region wherever that lies; it lands (dx, dy) away
                if (job.move_feather > 0.0f) {                          // a soft edge inside the selection: the feathered mask is the sprite's alpha
                    const rtdd_mask_refine f = {removal.select, RTDD_REFINE_FEATHER, 0, 0, -job.move_feather, 0.0f};
                    CK(rtdd_refine_mask(ctx, p_code, pi_code, rows, cols, &f, own.d_alpha, (size_t)cols));
                    CK(rtdd_lift_layer_matte(ctx, (uint8_t *)p_orig, pi_orig, own.d_alpha, (size_t)cols, rows, cols, 0, 0, own.d_msprite, w4, rows, cols));
                } else
                CK(rtdd_lift_layer(ctx, (uint8_t *)p_orig, pi_orig, p_code, pi_code, rows, cols, removal.select, 0, 0, own.d_msprite, w4, rows, cols));
                rtdd_layer L = {rows, cols, job.move_dx, job.move_dy, 256, RTDD_LAYER_NEAREST, 255, 0, 0, 0, 0, job.move_depth, job.move_depth, 0.0f};
                if (!job.move_has_depth) {
                    // keep the region's own depth, as one constant: the nearest d' of its pixels, read from a download of the map and the codes
                    std::vector<float> z((size_t)rows * cols); std::vector<unsigned char> code((size_t)rows * cols);
                    CK(rtdd_download(ctx, z.data(), w4, p_depth, pi_depth, w4, rows));
                    CK(rtdd_download(ctx, code.data(), cols, p_code, pi_code, cols, rows));
                    float nearest = 255.0f;
                    for (size_t i = 0; i < z.size(); i++)
                        if (removal.select == 0 ? code[i] != 0 : code[i] == removal.select) nearest = std::min(nearest, z[i] > 0.0f ? std::min(z[i], 255.0f) : 0.0f);
                    L.depth0 = L.depth1 = nearest;
                    if (n == 0) std::printf("move region %d by %d,%d at its own depth %g\n", job.removal.select, job.move_dx, job.move_dy, nearest);
                }
                CK(rtdd_composite_layer(ctx, own.d_rart, w3, own.d_rz, w4, own.d_msprite, w4, own.d_mart, w3, own.d_mz, w4, rows, cols, &L));
                r_orig = own.d_mart; r_depth = own.d_mz;
            }
        }
        const bool edited = job.has_layer || job.has_remove || job.has_move;
        void *const l_orig = job.has_layer ? (void *)own.d_lart : r_orig, *const l_depth = job.has_layer ? (void *)own.d_lz : r_depth;
        const size_t li_orig = job.has_layer ? (size_t)cols * 3 : ri_orig, li_depth = job.has_layer ? (size_t)cols * 4 : ri_depth;
        if (job.has_layer)
            CK(rtdd_composite_layer(ctx, (uint8_t *)r_orig, ri_orig, (float *)r_depth, ri_depth, own.d_sprite, (size_t)job.layer.cols * 4, own.d_lart, li_orig,
                                    own.d_lz, li_depth, rows, cols, &job.layer));
        {
        void *const p_orig = l_orig, *const p_depth = l_depth;          // (the names the effect calls below use)
        const size_t pi_orig = li_orig, pi_depth = li_depth;
        if (job.effect == "defocus") CK(rtdd_simulate_defocus(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols));
        else if (job.effect == "desaturation") CK(rtdd_simulate_desaturation(ctx, (uint8_t *)p_orig, pi_orig, (uint8_t *)p_gray, pi_gray, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols));
        else if (job.effect == "haze" && job.haze_ex)
            CK(rtdd_simulate_haze_ex(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, job.haze_beta,
                                     (uint8_t)job.air[0], (uint8_t)job.air[1], (uint8_t)job.air[2]));
        else if (job.effect == "haze") CK(rtdd_simulate_haze(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols));
        else if (job.effect == "refocus" && job.spread)
            CK(rtdd_simulate_bokeh(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, job.aperture,
                                   job.focus_depth, job.focus_x, job.focus_y));
        else if (job.effect == "refocus" && job.disc)
            CK(rtdd_simulate_lens_blur(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, job.aperture,
                                       job.focus_depth, job.focus_x, job.focus_y, RTDD_APERTURE_DISC));
        else if (job.effect == "refocus")
            CK(rtdd_simulate_refocus(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, job.aperture,
                                     job.focus_depth, job.focus_x, job.focus_y));
        else if (job.effect == "stereo")
            CK(rtdd_simulate_stereo(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, job.disparity,
                                    job.zero_depth, job.zero_x, job.zero_y, job.anaglyph ? RTDD_STEREO_ANAGLYPH : RTDD_STEREO_VIEW));
        else if (job.effect == "parallax") {
            const rtdd_parallax view = {job.shift_x, job.shift_y, job.dolly, job.zero_depth, job.zero_x, job.zero_y};
            const size_t w1 = (size_t)cols, w3 = w1 * 3, w4 = w1 * 4;
            if (job.has_plate) {                                        // the region taken out of the scene into the plate; the scene itself stays
                const uint8_t *p_code; size_t pi_code; rtdd_removal removal;
                CK(region_mask(ctx, job, own.d_sel, rows, cols, &p_code, &pi_code, &removal));
                CK(rtdd_remove_object(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, p_code, pi_code, own.d_part, w3, own.d_pplz, w4, rows, cols, &removal));
            }
            if (job.has_plate || own.d_pz || own.d_pcov)
                CK(rtdd_simulate_parallax_layered(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, own.d_part, w3, own.d_pplz, w4, (uint8_t *)p_art, pi_art,
                                                  own.d_pz, w4, own.d_pcov, w1, rows, cols, &view));
            else CK(rtdd_simulate_parallax(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &view));
            if (own.d_pz && parallax_files) {                           // the view's depth map as the harness writes every depth map: u8
                CK(rtdd_depth_to_u8(ctx, own.d_pz, w4, own.d_pz8, w1, rows, cols));
                parallax_files->depth_u8.resize((size_t)rows * cols);
                CK(rtdd_download(ctx, parallax_files->depth_u8.data(), w1, own.d_pz8, w1, w1, rows));
            }
            if (own.d_pcov && parallax_files) {
                parallax_files->coverage.resize((size_t)rows * cols);
                CK(rtdd_download(ctx, parallax_files->coverage.data(), w1, own.d_pcov, w1, w1, rows));
            }
        }
        else if (job.effect == "relight") {
            rtdd_light light = job.light;
            if (light.kind == RTDD_LIGHT_POINT) light.z = job.light_height;
            rtdd_ambient_occlusion ao = job.ao;
            ao.relief = light.relief;
            if (job.ao_lit) CK(rtdd_simulate_ambient_occlusion(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &ao, &light));
            else if (job.shadows) CK(rtdd_simulate_relight_shadowed(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &light, &job.shadow));
            else CK(rtdd_simulate_relight(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &light));
        }
        else if (job.effect == "lighting") {
            rtdd_light light = job.light;
            if (light.kind == RTDD_LIGHT_POINT) light.z = job.light_height;
            rtdd_shadow shadow = job.shadow;
            if (!job.shadows) shadow.maxSteps = 256;
            rtdd_ambient_occlusion ao = job.ao;
            ao.relief = light.relief;
            CK(rtdd_simulate_lighting(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &light, &shadow, &ao));
        }
        else if (job.effect == "ao") {
            rtdd_ambient_occlusion ao = job.ao;
            ao.relief = job.light.relief;
            CK(rtdd_simulate_ambient_occlusion(ctx, (uint8_t *)p_orig, pi_orig, (float *)p_depth, pi_depth, (uint8_t *)p_art, pi_art, rows, cols, &ao, nullptr));
        }
        }
        depth_u8->resize((size_t)rows * cols);
        CK(rtdd_download(ctx, depth_u8->data(), cols, p_u8, pi_u8, cols, rows));   // main.cpp:291 (synchronises)
        if (!job.effect.empty()) { art->resize((size_t)rows * cols * 3); CK(rtdd_download(ctx, art->data(), (size_t)cols * 3, p_art, pi_art, (size_t)cols * 3, rows)); }
        else if (edited) { art->resize((size_t)rows * cols * 3); CK(rtdd_download(ctx, art->data(), (size_t)cols * 3, l_orig, li_orig, (size_t)cols * 3, rows)); }     // no effect: the composite itself
        if (every_map) every_map->push_back(*depth_u8);                 // --write-all: the n-th estimate of this device
    }
    *ms_per_estimate = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (count > 0 ? count : 1);
    if (annotated) { annotated->resize((size_t)rows * cols * 3); CK(rtdd_download(ctx, annotated->data(), (size_t)cols * 3, p_ed, pi_ed, (size_t)cols * 3, rows)); }   // editedImage[0], main.cpp:298-303
    CK(rtdd_ctx_synchronize(ctx));                                      // (a persistent launch that gave up has been healed by now: include/rtdd.h RTDD_ERR_TIMEOUT)
    return RTDD_OK;
}

int main(int argc, const char *argv[]) {
    if (argc == 1) { std::printf("Usage: rtdd_harness -i image.(jpg|png|ppm) [-a annotation.(png|pgm)] [-o prefix] [--effect defocus|desaturation|haze|refocus|stereo|parallax|relight|ao|lighting] [--iters N] [--refine sor|mg|auto [--tolerance T]]\n"
                                 "                    [--focus D | --focus-at X,Y] [--aperture A] [--bokeh box|disc|spread] (refocus)  [--haze-beta B] [--airlight b,g,r] (haze)\n"
                                 "                    [--disparity D] [--zero-parallax Z | --zero-parallax-at X,Y] [--anaglyph] (stereo)\n"
                                 "                    --shift dx,dy [--dolly z] [--zero-parallax Z | --zero-parallax-at X,Y] [--plate-region id [--remove-grow N] [--remove-behind D]] [--parallax-depth-out FILE] [--parallax-coverage FILE] (parallax; --plate-region with --regions: the painted region removed into a background plate, rtdd_simulate_parallax_layered)\n"
                                 "                    [--light-dir x,y,z | --light-at X,Y [--light-height H] [--light-radius R]] [--relief S] [--ambient A] [--diffuse D] [--light-color b,g,r] (relight)\n"
                                 "                    [--shadows N [--shadow-bias B] [--shadow-softness S] [--shadow-strength T]] (relight with cast shadows)\n"
                                 "                    [--ao-radius R] [--ao-directions 4|8] [--ao-bias B] [--ao-strength T] [--relief S] [--ao-map] (ao)  [--ao R [--ao-directions ..] [--ao-bias ..] [--ao-strength ..]] (relight with its ambient term occluded)\n"
                                 "                    [relight's light flags] [--shadows N (256)] [--shadow-bias B] [--shadow-softness S] [--shadow-strength T] [--ao R (16)] [--ao-directions 4|8] [--ao-bias B] [--ao-strength T] (lighting: shade, cast shadows and occlusion in one call)\n"
                                 "                    [--layer sprite.(ppm|png|jpg) [--layer-alpha alpha.(pgm|png)] --layer-at x,y [--layer-scale S (256)] [--layer-filter nearest|bilinear] [--layer-depth z (128) | --layer-plane x0,y0,z0,x1,y1,z1] [--layer-feather f] [--layer-opacity o (255)]]   (a sprite inserted at a depth after the estimate, rtdd_composite_layer: --effect then runs on the composite and its depth map; without --effect ArtisticEffect is the composite)\n"
                                 "                    [--remove-region id [--remove-grow N (0..8)] [--remove-behind D] | --move-region id:dx,dy[:depth] [--remove-grow N] [--remove-behind D]]   (with --regions: the painted region taken out of the scene, rtdd_remove_object, or moved, rtdd_lift_layer + rtdd_remove_object + rtdd_composite_layer; before --layer and --effect, which run on the result and its depth map)\n"
                                 "                    [--select-grow R2 | --select-shrink R2] [--move-feather W]   (with --remove-region / --move-region / --plate-region: the region grown out to, or shrunk in by, the squared Euclidean distance R2 first, rtdd_refine_mask; with --move-region: a soft edge of W pixels, 0 < W <= 64, inside the moved selection, rtdd_lift_layer_matte)\n"
                                 "                    [--paint x,y,label,radius]... [--live N [--paint-at frame:x,y,label,radius]...] [--devices D --batch B [--sequential] [--write-all]] [--png] [--cold] [--edges gray|color] [--regions cut|smooth|both [--region-fill x,y;...:id]... [--region-wand x,y,tol:id]... [--surface-global] [--region-surface x,y,step[,below,above]:id]... [--segment step[,lo,hi[,minPixels[,maxRegions[,firstCode]]]]]]   (--segment: every surface of the ESTIMATED depth map at once, rtdd_segment_surfaces into the region pair behind the clicks, the largest as regions firstCode, firstCode + 1, ...; --region-surface: a click on the ESTIMATED depth map, rtdd_fill_surface into the region pair after the estimate and before --remove-region / --move-region / --plate-region; --surface-global: the clicks behind it take every pixel in their band; not with --live or --batch)\n"
                                 "                    [--stroke x0,y0,x1,y1,label,radius[,round]]... [--erase x0,y0,x1,y1,radius[,round]]...   (segments, in command-line order, one rtdd_paint_strokes call after --paint)\n"
                                 "                    [--ramp x0,y0,x1,y1,label0,label1,radius[,round]]...   (a depth ramp: label0 at x0,y0 to label1 at x1,y1; in order with --stroke / --erase, all of them one rtdd_paint_ramp_strokes call)\n"
                                 "                    [--fill \"x,y;x,y;...:label\" | \"x,y;...:label0,label1,ax0,ay0,ax1,ay1\"]... [--fill-erase \"x,y;x,y;...\"]... [--fill-rule nonzero|evenodd]   (a lasso filled with a label, a ramp along the axis, or erased: one rtdd_fill_polygon call each, after the strokes, in command-line order)\n"
                                 "                    [--wand \"x,y,tol:label\" | \"x,y,tol:label0,label1,ax0,ay0,ax1,ay1\"]... [--wand-erase \"x,y,tol\"]... [--wand-connect 4|8] [--wand-at frame:...]... [--wand-erase-at frame:...]...   (a click: everything joined to x,y within tol of its colour, one rtdd_fill_similar call each, after the polygons; -at: --live, in front of that frame)\n"
                                 "                    [--stroke-at frame:x0,y0,x1,y1,label,radius[,round]]... [--erase-at frame:x0,y0,x1,y1,radius[,round]]... [--ramp-at frame:x0,y0,x1,y1,label0,label1,radius[,round]]...   (--live: in front of that frame)\n"
                                 "       rtdd_harness --convert in.(jpg|png|ppm|pgm) out.(png|ppm|pgm)   (JPEG / 8-bit PNG / PNM -> PNG / PNM, no GPU)\n"); return 0; }
    if (argc == 4 && !std::strcmp(argv[1], "--convert")) {               // file format conversion only (no GPU): JPEG / PNG / PNM -> PNG / PNM
        Pnm im;
        if (!read_image(argv[2], im)) { std::printf("cannot read %s\n", argv[2]); return 2; }
        return write_image(argv[3], im.w, im.h, im.ch, im.px.data()) ? 0 : 5;
    }
    Job job;
    std::string in, an, out = "";
    bool png = false, write_all = false, shadow_opt = false, ao_opt = false, ao_radius_opt = false, layer_at = false, layer_opt = false, remove_opt = false;
    std::string layer_path, layer_alpha_path;
    int devices = 1, batch = 1, live = 0;
    int surface_flags = 0;                  // --surface-global: the --region-surface clicks behind it take every pixel in their band
    for (int i = 1; i < argc; i++) {
        auto next = [&]() -> const char * { return i + 1 < argc ? argv[++i] : ""; };
        if (!std::strcmp(argv[i], "-i")) in = next();
        else if (!std::strcmp(argv[i], "-a")) an = next();
        else if (!std::strcmp(argv[i], "-o")) out = next();
        else if (!std::strcmp(argv[i], "--effect")) job.effect = next();
        else if (!std::strcmp(argv[i], "--cold")) job.cold = true;
        else if (!std::strcmp(argv[i], "--edges")) {
            const char *v = next();
            if (!std::strcmp(v, "color")) job.edges_color = true;
            else if (std::strcmp(v, "gray")) { std::printf("--edges wants gray or color\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--regions")) {
            const char *v = next();
            job.region_flags = !std::strcmp(v, "cut") ? RTDD_REGION_CUT : !std::strcmp(v, "smooth") ? RTDD_REGION_SMOOTH : !std::strcmp(v, "both") ? RTDD_REGION_CUT | RTDD_REGION_SMOOTH : 0;
            if (!job.region_flags) { std::printf("--regions wants cut, smooth or both\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--region-fill")) {
            Job::Lasso l;
            if (!parse_fill(next(), false, job.fill_rule, &l) || l.fill.label0 != l.fill.label1) { std::printf("--region-fill wants x,y;x,y;...:id\n"); return 1; }
            job.region_fills.push_back(l);
        }
        else if (!std::strcmp(argv[i], "--surface-global")) surface_flags = RTDD_SURFACE_GLOBAL;
        else if (!std::strcmp(argv[i], "--segment")) {
            if (!parse_segment(next(), &job.segmentation)) { std::printf("--segment wants step[,lo,hi[,minPixels[,maxRegions[,firstCode]]]]\n"); return 1; }
            job.segment = true;
        }
        else if (!std::strcmp(argv[i], "--region-surface")) {
            rtdd_surface_wand w;
            if (!parse_surface(next(), surface_flags, &w) || w.label0 < 1 || w.label0 > 255) { std::printf("--region-surface wants x,y,step:id or x,y,step,below,above:id, the id 1..255\n"); return 1; }
            job.region_surfaces.push_back(w);
        }
        else if (!std::strcmp(argv[i], "--region-wand")) {
            Job::Wand q; q.frame = -1;
            if (!parse_wand(next(), false, job.wand_flags, &q.w, nullptr) || q.w.label0 != q.w.label1) { std::printf("--region-wand wants x,y,tol:id\n"); return 1; }
            job.region_wands.push_back(q);
        }
        else if (!std::strcmp(argv[i], "--iters")) job.iters = std::atoi(next());
        else if (!std::strcmp(argv[i], "--refine")) job.refine = next();          // sor | mg | auto
        else if (!std::strcmp(argv[i], "--tolerance")) job.tolerance = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--devices")) devices = std::atoi(next());
        else if (!std::strcmp(argv[i], "--batch")) batch = std::atoi(next());
        else if (!std::strcmp(argv[i], "--live")) live = std::atoi(next());
        else if (!std::strcmp(argv[i], "--sequential")) job.sequential = true;      // a --batch one estimate after the other (the round-4 behaviour)
        else if (!std::strcmp(argv[i], "--write-all")) write_all = true;           // every estimate of a --batch: <out>DepthMap_<b>.pgm|png
        else if (!std::strcmp(argv[i], "--png")) png = true;                       // DepthMap.png / ArtisticEffect.png like the reference
        else if (!std::strcmp(argv[i], "--paint")) { Paint p{0, 0, 0, 0, -1}; if (std::sscanf(next(), "%d,%d,%d,%d", &p.x, &p.y, &p.label, &p.radius) == 4) job.paints.push_back(p); }
        else if (!std::strcmp(argv[i], "--paint-at")) { Paint p{0, 0, 0, 0, 0}; if (std::sscanf(next(), "%d:%d,%d,%d,%d", &p.frame, &p.x, &p.y, &p.label, &p.radius) == 5) job.live_paints.push_back(p); }
        else if (!std::strcmp(argv[i], "--ramp") || !std::strcmp(argv[i], "--ramp-at")) {
            const bool at = argv[i][6] != 0; LiveStroke q; q.frame = -1;
            if (!parse_stroke(next(), 'r', &q.s, at ? &q.frame : nullptr)) { std::printf("%s\n", at ? "--ramp-at wants frame:x0,y0,x1,y1,label0,label1,radius[,round]" : "--ramp wants x0,y0,x1,y1,label0,label1,radius[,round]"); return 1; }
            if (at) job.live_strokes.push_back(q); else { job.strokes.push_back(q.s); job.has_ramp = true; }
        }
        else if (!std::strcmp(argv[i], "--fill-rule")) {
            const char *r = next();
            if (!std::strcmp(r, "nonzero")) job.fill_rule = RTDD_FILL_NONZERO;
            else if (!std::strcmp(r, "evenodd")) job.fill_rule = RTDD_FILL_EVEN_ODD;
            else { std::printf("--fill-rule wants nonzero or evenodd\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--fill") || !std::strcmp(argv[i], "--fill-erase")) {
            const bool erase = argv[i][6] != 0; Job::Lasso l;
            if (!parse_fill(next(), erase, job.fill_rule, &l)) { std::printf("%s\n", erase ? "--fill-erase wants x,y;x,y;..." : "--fill wants x,y;x,y;...:label or x,y;x,y;...:label0,label1,ax0,ay0,ax1,ay1"); return 1; }
            job.fills.push_back(l);
        }
        else if (!std::strcmp(argv[i], "--wand-connect")) {
            const char *v = next();
            if (!std::strcmp(v, "4")) job.wand_flags = 0;
            else if (!std::strcmp(v, "8")) job.wand_flags = RTDD_WAND_CONNECT_8;
            else { std::printf("--wand-connect wants 4 or 8\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--wand") || !std::strcmp(argv[i], "--wand-erase") || !std::strcmp(argv[i], "--wand-at") || !std::strcmp(argv[i], "--wand-erase-at")) {
            const bool erase = !std::strncmp(argv[i], "--wand-erase", 12), at = ends_with(argv[i], "-at"); Job::Wand q; q.frame = -1;
            if (!parse_wand(next(), erase, job.wand_flags, &q.w, at ? &q.frame : nullptr)) {
                std::printf("%s wants %sx,y,tolerance%s\n", argv[i - 1], at ? "frame:" : "", erase ? "" : ":label or ...:label0,label1,ax0,ay0,ax1,ay1"); return 1;
            }
            (at ? job.live_wands : job.wands).push_back(q);
        }
        else if (!std::strcmp(argv[i], "--stroke") || !std::strcmp(argv[i], "--erase")) {
            const bool erase = argv[i][2] == 'e'; rtdd_ramp_stroke q;
            if (!parse_stroke(next(), erase ? 'e' : 's', &q, nullptr)) { std::printf("%s\n", erase ? "--erase wants x0,y0,x1,y1,radius[,round]" : "--stroke wants x0,y0,x1,y1,label,radius[,round]"); return 1; }
            job.strokes.push_back(q);
        }
        else if (!std::strcmp(argv[i], "--stroke-at") || !std::strcmp(argv[i], "--erase-at")) {
            const bool erase = argv[i][2] == 'e'; LiveStroke q;
            if (!parse_stroke(next(), erase ? 'e' : 's', &q.s, &q.frame)) { std::printf("%s\n", erase ? "--erase-at wants frame:x0,y0,x1,y1,radius[,round]" : "--stroke-at wants frame:x0,y0,x1,y1,label,radius[,round]"); return 1; }
            job.live_strokes.push_back(q);
        }
        else if (!std::strcmp(argv[i], "--focus")) { job.focus_depth = (float)std::atof(next()); job.focus_x = -1; }
        else if (!std::strcmp(argv[i], "--focus-at")) { if (std::sscanf(next(), "%d,%d", &job.focus_x, &job.focus_y) != 2) { std::printf("--focus-at wants X,Y\n"); return 1; } }
        else if (!std::strcmp(argv[i], "--aperture")) job.aperture = std::atof(next());
        else if (!std::strcmp(argv[i], "--bokeh")) {
            const std::string b = next();
            if (b != "box" && b != "disc" && b != "spread") { std::printf("--bokeh wants box or disc or spread\n"); return 1; }
            job.disc = b == "disc"; job.spread = b == "spread";
        }
        else if (!std::strcmp(argv[i], "--disparity")) job.disparity = std::atoi(next());
        else if (!std::strcmp(argv[i], "--zero-parallax")) { job.zero_depth = (float)std::atof(next()); job.zero_x = -1; }
        else if (!std::strcmp(argv[i], "--zero-parallax-at")) { if (std::sscanf(next(), "%d,%d", &job.zero_x, &job.zero_y) != 2) { std::printf("--zero-parallax-at wants X,Y\n"); return 1; } }
        else if (!std::strcmp(argv[i], "--anaglyph")) job.anaglyph = true;
        else if (!std::strcmp(argv[i], "--shift")) { if (std::sscanf(next(), "%d,%d", &job.shift_x, &job.shift_y) != 2) { std::printf("--shift wants dx,dy\n"); return 1; } }
        else if (!std::strcmp(argv[i], "--dolly")) job.dolly = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--light-dir")) {
            if (std::sscanf(next(), "%f,%f,%f", &job.light.x, &job.light.y, &job.light.z) != 3) { std::printf("--light-dir wants x,y,z\n"); return 1; }
            job.light.kind = RTDD_LIGHT_DIRECTIONAL;
        }
        else if (!std::strcmp(argv[i], "--light-at")) {
            if (std::sscanf(next(), "%d,%d", &job.light.anchorX, &job.light.anchorY) != 2) { std::printf("--light-at wants X,Y\n"); return 1; }
            job.light.kind = RTDD_LIGHT_POINT; job.light.x = (float)job.light.anchorX; job.light.y = (float)job.light.anchorY;
        }
        else if (!std::strcmp(argv[i], "--light-height")) job.light_height = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--light-radius")) job.light.radius = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--relief")) job.light.relief = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--shadows")) { job.shadow.maxSteps = std::atoi(next()); job.shadows = true; }
        else if (!std::strcmp(argv[i], "--shadow-bias")) { job.shadow.bias = (float)std::atof(next()); shadow_opt = true; }
        else if (!std::strcmp(argv[i], "--shadow-softness")) { job.shadow.softness = (float)std::atof(next()); shadow_opt = true; }
        else if (!std::strcmp(argv[i], "--shadow-strength")) { job.shadow.strength = (float)std::atof(next()); shadow_opt = true; }
        else if (!std::strcmp(argv[i], "--ao")) { job.ao.radius = std::atoi(next()); job.ao_lit = true; }
        else if (!std::strcmp(argv[i], "--ao-radius")) { job.ao.radius = std::atoi(next()); ao_radius_opt = true; }
        else if (!std::strcmp(argv[i], "--ao-directions")) { job.ao.directions = std::atoi(next()); ao_opt = true; }
        else if (!std::strcmp(argv[i], "--ao-bias")) { job.ao.bias = (float)std::atof(next()); ao_opt = true; }
        else if (!std::strcmp(argv[i], "--ao-strength")) { job.ao.strength = (float)std::atof(next()); ao_opt = true; }
        else if (!std::strcmp(argv[i], "--ao-map")) { job.ao.mode = RTDD_AO_MAP; ao_radius_opt = true; }
        else if (!std::strcmp(argv[i], "--ambient")) job.light.ambient = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--diffuse")) job.light.diffuse = (float)std::atof(next());
        else if (!std::strcmp(argv[i], "--light-color")) {
            int c[3];
            if (std::sscanf(next(), "%d,%d,%d", &c[0], &c[1], &c[2]) != 3) { std::printf("--light-color wants b,g,r\n"); return 1; }
            for (int k = 0; k < 3; k++) if (c[k] < 0 || c[k] > 255) { std::printf("--light-color: each of b,g,r must be 0..255\n"); return 1; }
            job.light.colorB = (uint8_t)c[0]; job.light.colorG = (uint8_t)c[1]; job.light.colorR = (uint8_t)c[2];
        }
        else if (!std::strcmp(argv[i], "--remove-region")) { job.removal.select = std::atoi(next()); job.has_remove = true; }
        else if (!std::strcmp(argv[i], "--plate-region")) { job.removal.select = std::atoi(next()); job.has_plate = true; }
        else if (!std::strcmp(argv[i], "--parallax-depth-out")) job.parallax_depth_out = next();
        else if (!std::strcmp(argv[i], "--parallax-coverage")) job.parallax_coverage = next();
        else if (!std::strcmp(argv[i], "--remove-grow")) { job.removal.grow = std::atoi(next()); remove_opt = true; }
        else if (!std::strcmp(argv[i], "--remove-behind")) { job.removal.sourceMinDepth = (float)std::atof(next()); remove_opt = true; }
        else if (!std::strcmp(argv[i], "--move-region")) {
            const int got = std::sscanf(next(), "%d:%d,%d:%f", &job.removal.select, &job.move_dx, &job.move_dy, &job.move_depth);
            if (got < 3) { std::printf("--move-region wants id:dx,dy or id:dx,dy:depth\n"); return 1; }
            job.move_has_depth = got == 4; job.has_move = true;
        }
        else if (!std::strcmp(argv[i], "--select-grow") || !std::strcmp(argv[i], "--select-shrink")) {
            if (job.select_op >= 0) { std::printf("--select-grow and --select-shrink: one at a time\n"); return 1; }
            job.select_op = argv[i][9] == 'g' ? RTDD_REFINE_GROW : RTDD_REFINE_SHRINK; job.select_r2 = std::atoi(next());
            if (job.select_r2 < 1 || job.select_r2 > 1024 * 1024) { std::printf("--select-grow and --select-shrink want a squared radius, 1..1048576\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--move-feather")) {
            job.move_feather = (float)std::atof(next());
            if (!(job.move_feather > 0.0f && job.move_feather <= 64.0f)) { std::printf("--move-feather wants a width W, 0 < W <= 64\n"); return 1; }
        }
        else if (!std::strcmp(argv[i], "--layer")) layer_path = next();
        else if (!std::strcmp(argv[i], "--layer-alpha")) { layer_alpha_path = next(); layer_opt = true; }
        else if (!std::strcmp(argv[i], "--layer-at")) { if (std::sscanf(next(), "%d,%d", &job.layer.x, &job.layer.y) != 2) { std::printf("--layer-at wants x,y\n"); return 1; } layer_at = layer_opt = true; }
        else if (!std::strcmp(argv[i], "--layer-scale")) { job.layer.scale = std::atoi(next()); layer_opt = true; }
        else if (!std::strcmp(argv[i], "--layer-filter")) {
            const char *v = next();
            if (!std::strcmp(v, "bilinear")) job.layer.filter = RTDD_LAYER_BILINEAR;
            else if (std::strcmp(v, "nearest")) { std::printf("--layer-filter wants nearest or bilinear\n"); return 1; }
            layer_opt = true;
        }
        else if (!std::strcmp(argv[i], "--layer-depth")) { job.layer.depth0 = job.layer.depth1 = (float)std::atof(next()); job.layer.x0 = job.layer.y0 = job.layer.x1 = job.layer.y1 = 0; layer_opt = true; }
        else if (!std::strcmp(argv[i], "--layer-plane")) {
            rtdd_layer &q = job.layer;
            if (std::sscanf(next(), "%d,%d,%f,%d,%d,%f", &q.x0, &q.y0, &q.depth0, &q.x1, &q.y1, &q.depth1) != 6) { std::printf("--layer-plane wants x0,y0,z0,x1,y1,z1\n"); return 1; }
            layer_opt = true;
        }
        else if (!std::strcmp(argv[i], "--layer-feather")) { job.layer.feather = (float)std::atof(next()); layer_opt = true; }
        else if (!std::strcmp(argv[i], "--layer-opacity")) { job.layer.opacity = std::atoi(next()); layer_opt = true; }
        else if (!std::strcmp(argv[i], "--haze-beta")) { job.haze_beta = (float)std::atof(next()); job.haze_ex = true; }
        else if (!std::strcmp(argv[i], "--airlight")) {
            if (std::sscanf(next(), "%d,%d,%d", &job.air[0], &job.air[1], &job.air[2]) != 3) { std::printf("--airlight wants b,g,r\n"); return 1; }
            for (int c = 0; c < 3; c++) if (job.air[c] < 0 || job.air[c] > 255) { std::printf("--airlight: each of b,g,r must be 0..255\n"); return 1; }
            job.haze_ex = true;
        }
        else if (!std::strcmp(argv[i], "-h")) std::printf("Usage:\n -i input image (JPEG, 8-bit PNG, binary PPM)\n -a annotated image (8-bit PNG, binary PGM)\n");
    }
    // cast shadows belong to relight, and their parameters to --shadows: a stray one is refused, not dropped
    const bool lighting = job.effect == "lighting";                           // takes --shadows and --ao together, each with its parameters
    if (job.shadows && job.effect != "relight" && !lighting) { std::printf("--shadows needs --effect relight\n"); return 1; }
    if (job.region_flags == 0 && (!job.region_fills.empty() || !job.region_wands.empty())) { std::printf("--region-fill and --region-wand need --regions cut|smooth|both\n"); return 1; }
    if (!job.region_surfaces.empty() && job.region_flags == 0) { std::printf("--region-surface needs --regions cut|smooth|both\n"); return 1; }
    if (!job.region_surfaces.empty() && (live > 0 || batch > 1)) { std::printf("--region-surface is not supported with --live or --batch\n"); return 1; }
    if (job.segment && job.region_flags == 0) { std::printf("--segment needs --regions cut|smooth|both\n"); return 1; }
    if (job.segment && (live > 0 || batch > 1)) { std::printf("--segment is not supported with --live or --batch\n"); return 1; }
    if (shadow_opt && !job.shadows && !lighting) { std::printf("--shadow-bias, --shadow-softness and --shadow-strength need --shadows N\n"); return 1; }
    // ambient occlusion is --effect ao, or --ao R under --effect relight (without cast shadows: one call renders one or the other); its
    // parameters belong to one of the two: a stray one is refused, not dropped
    if (job.ao_lit && job.effect != "relight" && !lighting) { std::printf("--ao needs --effect relight (without a light: --effect ao --ao-radius R)\n"); return 1; }
    if (job.ao_lit && job.shadows && !lighting) { std::printf("--ao and --shadows cannot be combined: ambient occlusion and cast shadows are separate calls (both in one call: --effect lighting)\n"); return 1; }
    if (ao_radius_opt && job.effect != "ao") { std::printf("--ao-radius and --ao-map need --effect ao (under --effect relight: --ao R)\n"); return 1; }
    if (ao_opt && !job.ao_lit && job.effect != "ao" && !lighting) { std::printf("--ao-directions, --ao-bias and --ao-strength need --ao R or --effect ao\n"); return 1; }
    // a live frame's sticky effect is an effect code without parameters (rtdd_live_submit_ex): the aimed effects are not available there
    if (live > 0 && (job.effect == "refocus" || job.effect == "stereo" || job.effect == "parallax" || job.effect == "relight" || job.effect == "ao" || lighting || (job.effect == "haze" && job.haze_ex))) {
        std::printf("--live renders the reference's three effects only: --effect refocus, --effect stereo, --effect parallax, --effect relight, --effect ao, --effect lighting and --haze-beta / --airlight are not supported with --live\n");
        return 1;
    }
    // a layer is a sprite and where it lands; its parameters belong to it: a stray one is refused, not dropped.  A live frame renders no layer
    if (layer_opt && layer_path.empty()) { std::printf("--layer-alpha, --layer-at, --layer-scale, --layer-filter, --layer-depth, --layer-plane, --layer-feather and --layer-opacity need --layer sprite\n"); return 1; }
    if (!layer_path.empty() && !layer_at) { std::printf("--layer needs --layer-at x,y\n"); return 1; }
    if (live > 0 && !layer_path.empty()) { std::printf("--layer is not supported with --live\n"); return 1; }
    // a removal works on a painted region: its flags belong to it, it needs the regions, and one of the two forms at a time
    if (remove_opt && !job.has_remove && !job.has_move && !job.has_plate) { std::printf("--remove-grow and --remove-behind need --remove-region id, --move-region id:dx,dy or --plate-region id\n"); return 1; }
    if (job.select_op >= 0 && !job.has_remove && !job.has_move && !job.has_plate) { std::printf("--select-grow and --select-shrink need --remove-region id, --move-region id:dx,dy or --plate-region id\n"); return 1; }
    if (job.move_feather > 0.0f && !job.has_move) { std::printf("--move-feather needs --move-region id:dx,dy\n"); return 1; }
    if ((job.select_op >= 0 || job.move_feather > 0.0f) && (live > 0 || batch > 1)) { std::printf("--select-grow, --select-shrink and --move-feather are not supported with --live or --batch\n"); return 1; }
    // the two-layer parallax view: a plate is a painted region removed for --effect parallax alone; one removal per run
    const bool parallax_out = !job.parallax_depth_out.empty() || !job.parallax_coverage.empty();
    if (live > 0 && (job.has_plate || parallax_out)) { std::printf("--plate-region, --parallax-depth-out and --parallax-coverage are not supported with --live\n"); return 1; }
    if ((job.has_plate || parallax_out) && job.effect != "parallax") { std::printf("--plate-region, --parallax-depth-out and --parallax-coverage need --effect parallax\n"); return 1; }
    if (job.has_plate && (job.has_remove || job.has_move)) { std::printf("--plate-region cannot be combined with --remove-region or --move-region\n"); return 1; }
    if (job.has_plate && job.region_flags == 0) { std::printf("--plate-region needs --regions cut|smooth|both and a painted region\n"); return 1; }
    if (job.has_plate && (job.removal.select < 1 || job.removal.select > 255)) { std::printf("a region id is 1..255\n"); return 1; }
    if (job.has_remove && job.has_move) { std::printf("--remove-region and --move-region: one at a time\n"); return 1; }
    if (live > 0 && (job.has_remove || job.has_move)) { std::printf("--remove-region and --move-region are not supported with --live\n"); return 1; }
    if ((job.has_remove || job.has_move) && job.region_flags == 0) { std::printf("--remove-region and --move-region need --regions cut|smooth|both and a painted region\n"); return 1; }
    if ((job.has_remove || job.has_move) && (job.removal.select < 1 || job.removal.select > 255)) { std::printf("a region id is 1..255\n"); return 1; }
    if (!layer_path.empty()) {
        Pnm s, a;
        if (!read_image(layer_path, s) || s.ch != 3) { std::printf("cannot read %s as a colour image (binary PPM, 8-bit PNG or JPEG)\n", layer_path.c_str()); return 2; }
        if (!layer_alpha_path.empty() && (!read_image(layer_alpha_path, a) || a.ch != 1 || a.w != s.w || a.h != s.h)) { std::printf("cannot read %s as a gray image of the sprite's size\n", layer_alpha_path.c_str()); return 2; }
        job.layer.rows = s.h; job.layer.cols = s.w;
        job.sprite.resize((size_t)s.w * s.h * 4);
        for (size_t i = 0; i < (size_t)s.w * s.h; i++) {                     // the file is RGB; no --layer-alpha: opaque
            job.sprite[4 * i] = s.px[3 * i + 2]; job.sprite[4 * i + 1] = s.px[3 * i + 1]; job.sprite[4 * i + 2] = s.px[3 * i];
            job.sprite[4 * i + 3] = layer_alpha_path.empty() ? 255 : a.px[i];
        }
        job.has_layer = true;
    }
    Pnm rgb;
    if (!read_image(in, rgb)) { std::printf("cannot read %s as a binary PPM / PGM, an 8-bit PNG or a JPEG\n", in.c_str()); return 2; }
    if (rgb.ch == 1) {                                                       // cv::imread's default flag gives three channels whatever the file holds
        Pnm c; c.w = rgb.w; c.h = rgb.h; c.ch = 3; c.px.resize(rgb.px.size() * 3);
        for (size_t i = 0; i < rgb.px.size(); i++) c.px[3 * i] = c.px[3 * i + 1] = c.px[3 * i + 2] = rgb.px[i];
        rgb = c;
    }
    job.bgr = rgb;
    for (size_t i = 0; i < rgb.px.size(); i += 3) { job.bgr.px[i] = rgb.px[i + 2]; job.bgr.px[i + 2] = rgb.px[i]; }   // cv::imread gives BGR
    if (!an.empty()) {
        if (!read_image(an, job.ann) || job.ann.w != rgb.w || job.ann.h != rgb.h) { std::printf("cannot read %s as a binary PGM / 8-bit PNG of the image's size\n", an.c_str()); return 2; }
        if (job.ann.ch == 3) {                                               // cv::imread(path, 0) of a colour file: BT.601 gray, as for the image
            Pnm g1; g1.w = job.ann.w; g1.h = job.ann.h; g1.ch = 1; g1.px.resize((size_t)g1.w * g1.h);
            for (size_t i = 0; i < g1.px.size(); i++) g1.px[i] = (unsigned char)((job.ann.px[3 * i] * 4899 + job.ann.px[3 * i + 1] * 9617 + job.ann.px[3 * i + 2] * 1868 + 8192) >> 14);
            job.ann = g1;
        }
        job.has_ann = true;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::printf("no HIP device: %s\n", rtdd_status_string(RTDD_ERR_NO_DEVICE)); return 3; }
    if (devices > ndev) devices = ndev;

    std::vector<std::vector<unsigned char>> depth(devices), art(devices), annotated(devices);
    std::vector<std::vector<std::vector<unsigned char>>> every(devices);   // [device][n-th estimate on it]: image b = n * devices + device
    std::vector<double> ms(devices, 0.0);
    std::vector<int> rcs(devices, 0), counts(devices, 0);
    for (int b = 0; b < batch; b++) counts[b % devices]++;               // image b -> device b % D
    if (live > 0) { counts.assign(devices, 0); counts[0] = live; }
    auto t0 = std::chrono::steady_clock::now();
    ParallaxFiles parallax_files;
    std::vector<std::thread> th;
    for (int d = 0; d < devices; d++)
        th.emplace_back([&, d]() { rcs[d] = counts[d] ? run_device(d, job, counts[d], live > 0, &depth[d], &art[d], &ms[d], write_all ? &every[d] : nullptr, d == 0 ? &annotated[0] : nullptr, d == 0 ? &parallax_files : nullptr) : 0; });
    for (auto &t : th) t.join();
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int d = 0; d < devices; d++) if (rcs[d]) return 4;

    const int total = live > 0 ? live : batch;
    // (the reference's clock() brackets the FIRST estimate of the process, first-call costs included: that figure is --cold's; the default
    // runs a warm-up estimate and the three effects on a throw-away context first, so that what is printed is the steady cost)
    std::printf("Processing Time: %.3f ms per estimate on device 0 (upload + estimate%s + download; %s); %d estimate(s) on %d device(s) in %.1f ms wall incl. setup\n",
                ms[0], job.effect.empty() ? "" : " + effect",
                job.cold ? "COLD: the process's first estimate, first-call costs included, like the reference's clock()" : "WARM: after a warm-up on a throw-away context; --cold for the first-call figure",
                total, devices, wall);
    if (live > 0 && job.refine.empty())
        std::printf("Live: %.1f frames/s (%d frames, annotation upload + estimate%s + map download per frame, two frames in flight)\n", 1e3 / (ms[0] > 0 ? ms[0] : 1), live,
                    job.effect.empty() ? "" : " + sticky effect and its image's download");
    if (!write_image(out + (png ? "DepthMap.png" : "DepthMap.pgm"), rgb.w, rgb.h, 1, depth[0].data())) { std::printf("cannot write %sDepthMap\n", out.c_str()); return 5; }
    {                                                                    // main.cpp:298-303: editedImage[0] -- the image with the scribbles in it
        std::vector<unsigned char> o(annotated[0]);
        for (size_t i = 0; i + 2 < o.size(); i += 3) { o[i] = annotated[0][i + 2]; o[i + 2] = annotated[0][i]; }     // BGR -> RGB for the file
        if (!o.empty() && !write_image(out + (png ? "AnnotatedImage.png" : "AnnotatedImage.ppm"), rgb.w, rgb.h, 3, o.data())) return 5;
    }
    if (!job.effect.empty() || job.has_layer || job.has_remove || job.has_move) {     // (--layer, --remove-region or --move-region without --effect: their result)
        std::vector<unsigned char> o(art[0]);
        for (size_t i = 0; i < o.size(); i += 3) { o[i] = art[0][i + 2]; o[i + 2] = art[0][i]; }     // BGR -> RGB for the file
        if (!write_image(out + (png ? "ArtisticEffect.png" : "ArtisticEffect.ppm"), rgb.w, rgb.h, 3, o.data())) return 5;
    }
    if (!job.parallax_depth_out.empty() && !write_image(job.parallax_depth_out, rgb.w, rgb.h, 1, parallax_files.depth_u8.data())) { std::printf("cannot write %s\n", job.parallax_depth_out.c_str()); return 5; }
    if (!job.parallax_coverage.empty() && !write_image(job.parallax_coverage, rgb.w, rgb.h, 1, parallax_files.coverage.data())) { std::printf("cannot write %s\n", job.parallax_coverage.c_str()); return 5; }
    if (write_all)
        for (int d = 0; d < devices; d++)
            for (size_t n = 0; n < every[d].size(); n++) {
                const std::string name = out + "DepthMap_" + std::to_string(n * devices + d) + (png ? ".png" : ".pgm");
                if (!write_image(name, rgb.w, rgb.h, 1, every[d][n].data())) { std::printf("cannot write %s\n", name.c_str()); return 5; }
            }
    std::printf("Saving images...\n");                                   // main.cpp:317
    return 0;
}
