// tc2li_image_prep_* / tc2li_host_image_prep_batch (include/tc2li_hip.h "image ingest"): the clone / cv::remap / cv::resize of
// System::TrackStereoLidar (SF/src/System.cc:240-257) and the cvtColor of Tracking::GrabImageStereoLidar (SF/src/Tracking.cc:1646-1671).
// This file validates the calls, keeps the handle (the fixed-point maps, the resize tables, the staging of host images) and runs the
// host twin: plain C++ on the worker pool with the arithmetic of image_prep_device.hpp, the same the kernels run.
#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "image_prep_device.hpp"
#include "orb_device.hpp"

struct tc2li_image_prep {
    tc2li_image_prep_params prm;
    int max_images = 0;
    std::mutex mu;
    bool maps_set[2] = {false, false};
    int rec_pitch = 0;
    tc2li::DevBuf<uint32_t> rec_xy[2];
    tc2li::DevBuf<uint16_t> rec_frac[2];
    tc2li::DevBuf<float> map_stage;            // the float maps of one camera on their way to k_prep_fix_maps
    tc2li::DevBuf<int> xofs, yofs;             // RESIZE
    tc2li::DevBuf<short> ialpha, ibeta;
    tc2li::DevBuf<uint8_t> stage;              // host images of a call
    tc2li::PinnedBuf<uint8_t> h_stage;
    hipEvent_t records_read = nullptr;         // RECTIFY: behind the last queued kernel that reads the records; set_maps waits for it
    bool records_in_use = false;
    ~tc2li_image_prep() { if (records_read) (void)hipEventDestroy(records_read); }
};

namespace tc2li {
namespace {

int validate_params(const char* entry, const tc2li_image_prep_params* p) {
    if (!p) { set_error("%s: null params", entry); return TC2LI_ERR_INVALID; }
    if (p->channels != 1 && p->channels != 3 && p->channels != 4) {
        set_error("%s: %d channels (1, 3 or 4)", entry, p->channels);
        return TC2LI_ERR_INVALID;
    }
    const int dims[4] = {p->src_width, p->src_height, p->dst_width, p->dst_height};
    for (int d : dims)
        if (d < 1 || d > kImagePrepMaxDim) {
            set_error("%s: a dimension of %d (1 .. %d)", entry, d, kImagePrepMaxDim);
            return TC2LI_ERR_INVALID;
        }
    if (p->mode != TC2LI_IMAGE_PREP_COPY && p->mode != TC2LI_IMAGE_PREP_RECTIFY && p->mode != TC2LI_IMAGE_PREP_RESIZE) {
        set_error("%s: unknown mode %d", entry, p->mode);
        return TC2LI_ERR_INVALID;
    }
    if (p->mode == TC2LI_IMAGE_PREP_COPY && (p->dst_width != p->src_width || p->dst_height != p->src_height)) {
        set_error("%s: mode COPY with a destination size other than the source's", entry);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

size_t image_bytes(int rows, int stride, int row_bytes) { return (size_t)(rows - 1) * (size_t)stride + (size_t)row_bytes; }

int validate_call(const char* entry, const tc2li_image_prep_params& p, const uint8_t* images, int n_images, int stride, const uint8_t* gray,
                  int gray_stride, size_t gray_pitch_bytes) {
    if (n_images < 0 || (n_images && (!images || !gray))) { set_error("%s: null or negative argument", entry); return TC2LI_ERR_INVALID; }
    if ((long long)stride < (long long)p.src_width * p.channels) {
        set_error("%s: stride %d below width * channels = %d", entry, stride, p.src_width * p.channels);
        return TC2LI_ERR_INVALID;
    }
    if (gray_stride < p.dst_width) { set_error("%s: gray_stride %d below dst_width %d", entry, gray_stride, p.dst_width); return TC2LI_ERR_INVALID; }
    if (n_images > 1 && gray_pitch_bytes < image_bytes(p.dst_height, gray_stride, p.dst_width)) {
        set_error("%s: gray_pitch_bytes %zu: the gray images would overlap", entry, gray_pitch_bytes);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

// a map of w x h floats: every value finite and below 2^24 in magnitude (cvRound is undefined beyond)
bool map_ok(const float* m, int w, int h) {
    std::vector<uint8_t> bad((size_t)h, 0);
    global_pool().parallel_for(h, [&](int y) {
        const float* row = m + (size_t)y * w;
        bool ok = true;
        for (int x = 0; x < w; ++x) ok &= prep::map_value_ok(row[x]);
        bad[y] = !ok;
    });
    return std::find(bad.begin(), bad.end(), 1) == bad.end();
}

struct HostJob {
    const tc2li_image_prep_params* p;
    const float* const* maps;
    const uint8_t* images;
    size_t image_pitch;
    int stride;
    uint8_t* gray;
    size_t gray_pitch;
    int gray_stride;
    int k0, k2, nc;                            // nc: the channels that are read
    std::vector<int> xofs, yofs;
    std::vector<short> ialpha, ibeta;
};

inline uint8_t finish(const int* v, int nc, int k0, int k2) { return (uint8_t)(nc == 1 ? v[0] : prep::gray(v[0], v[1], v[2], k0, k2)); }

void host_row(const HostJob& J, int img, int y) {
    const tc2li_image_prep_params& p = *J.p;
    const int C = p.channels, nc = J.nc, sw = p.src_width, sh = p.src_height;
    const uint8_t* S = J.images + (size_t)img * J.image_pitch;
    uint8_t* D = J.gray + (size_t)img * J.gray_pitch + (size_t)y * J.gray_stride;
    int v[3] = {0, 0, 0};
    if (p.mode == TC2LI_IMAGE_PREP_COPY) {
        const uint8_t* R = S + (size_t)y * J.stride;
        for (int x = 0; x < p.dst_width; ++x) {
            for (int c = 0; c < nc; ++c) v[c] = R[(size_t)x * C + c];
            D[x] = finish(v, nc, J.k0, J.k2);
        }
    } else if (p.mode == TC2LI_IMAGE_PREP_RECTIFY) {
        const float* mx = J.maps[2 * (img & 1)] + (size_t)y * p.dst_width;
        const float* my = J.maps[2 * (img & 1) + 1] + (size_t)y * p.dst_width;
        auto tap = [&](int ty, int tx, int c) -> int {   // BORDER_CONSTANT 0
            return ty >= 0 && ty < sh && tx >= 0 && tx < sw ? S[(size_t)ty * J.stride + (size_t)tx * C + c] : 0;
        };
        for (int x = 0; x < p.dst_width; ++x) {
            int ix, iy, frac;
            prep::fix_map(mx[x], my[x], &ix, &iy, &frac);
            for (int c = 0; c < nc; ++c) v[c] = prep::remap_blend(tap(iy, ix, c), tap(iy, ix + 1, c), tap(iy + 1, ix, c), tap(iy + 1, ix + 1, c), frac);
            D[x] = finish(v, nc, J.k0, J.k2);
        }
    } else {
        const int sy0 = std::min(std::max(J.yofs[y], 0), sh - 1), sy1 = std::min(std::max(J.yofs[y] + 1, 0), sh - 1);
        const uint8_t* R0 = S + (size_t)sy0 * J.stride;
        const uint8_t* R1 = S + (size_t)sy1 * J.stride;
        const int b0 = J.ibeta[2 * y], b1 = J.ibeta[2 * y + 1];
        for (int x = 0; x < p.dst_width; ++x) {
            const int sx = J.xofs[x], sx1 = std::min(sx + 1, sw - 1), a0 = J.ialpha[2 * x], a1 = J.ialpha[2 * x + 1];
            for (int c = 0; c < nc; ++c)
                v[c] = prep::resize_combine(prep::resize_row(R0[(size_t)sx * C + c], R0[(size_t)sx1 * C + c], a0, a1),
                                            prep::resize_row(R1[(size_t)sx * C + c], R1[(size_t)sx1 * C + c], a0, a1), b0, b1);
            D[x] = finish(v, nc, J.k0, J.k2);
        }
    }
}

constexpr int kHostRowsPerUnit = 16;

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_image_prep_create(const tc2li_image_prep_params* params, int max_images, tc2li_image_prep** out) {
    if (!out) { set_error("tc2li_image_prep_create: null out"); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    const int rc = validate_params("tc2li_image_prep_create", params);
    if (rc < 0) return rc;
    if (max_images < 1 || max_images > kImagePrepMaxImages) {
        set_error("tc2li_image_prep_create: max_images %d (1 .. %d)", max_images, kImagePrepMaxImages);
        return TC2LI_ERR_INVALID;
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    std::unique_ptr<tc2li_image_prep> h(new tc2li_image_prep());
    h->prm = *params;
    h->max_images = max_images;
    const int dw = params->dst_width, dh = params->dst_height;
    if (params->mode == TC2LI_IMAGE_PREP_RECTIFY) {
        h->rec_pitch = (dw + 3) & ~3;
        for (int cam = 0; cam < 2; ++cam) {
            TC2LI_HIP_CHECK(h->rec_xy[cam].alloc((size_t)h->rec_pitch * dh));
            TC2LI_HIP_CHECK(h->rec_frac[cam].alloc((size_t)h->rec_pitch * dh));
        }
        TC2LI_HIP_CHECK(h->map_stage.alloc(2 * (size_t)dw * dh));
        TC2LI_HIP_CHECK(hipEventCreateWithFlags(&h->records_read, hipEventDisableTiming));
    } else if (params->mode == TC2LI_IMAGE_PREP_RESIZE) {
        std::vector<int> xofs, yofs;
        std::vector<short> ia, ib;
        build_resize_tables(params->src_width, params->src_height, dw, dh, xofs, ia, yofs, ib);
        xofs.resize((size_t)(dw + 3) & ~(size_t)3, 0);          // k_prep_resize loads the columns' entries four at a time
        ia.resize(2 * ((size_t)(dw + 3) & ~(size_t)3), 0);
        TC2LI_HIP_CHECK(h->xofs.upload(xofs));
        TC2LI_HIP_CHECK(h->yofs.upload(yofs));
        TC2LI_HIP_CHECK(h->ialpha.upload(ia));
        TC2LI_HIP_CHECK(h->ibeta.upload(ib));
    }
    *out = h.release();
    return TC2LI_OK;
}

extern "C" void tc2li_image_prep_destroy(tc2li_image_prep* prep) { delete prep; }

extern "C" int tc2li_image_prep_set_maps(tc2li_image_prep* prep, int camera, const float* map_x, const float* map_y, void* stream) {
    if (!prep || !map_x || !map_y || (camera != 0 && camera != 1)) {
        set_error("tc2li_image_prep_set_maps: null argument or a camera other than 0 / 1");
        return TC2LI_ERR_INVALID;
    }
    if (prep->prm.mode != TC2LI_IMAGE_PREP_RECTIFY) { set_error("tc2li_image_prep_set_maps: the handle's mode is not RECTIFY"); return TC2LI_ERR_INVALID; }
    const int w = prep->prm.dst_width, h = prep->prm.dst_height;
    if (!map_ok(map_x, w, h) || !map_ok(map_y, w, h)) {
        set_error("tc2li_image_prep_set_maps: camera %d: a map value that is not finite or not below 2^24 in magnitude", camera);
        return TC2LI_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(prep->mu);
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    const size_t n = (size_t)w * h;
    // a batch call on device images only queues its kernel: the records are not overwritten before it has read them
    if (prep->records_in_use) TC2LI_HIP_CHECK(hipStreamWaitEvent(st, prep->records_read, 0));
    prep->maps_set[camera] = false;
    TC2LI_HIP_CHECK(hipMemcpyAsync(prep->map_stage.p, map_x, n * sizeof(float), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(prep->map_stage.p + n, map_y, n * sizeof(float), hipMemcpyHostToDevice, st));
    launch_image_prep_fix_maps(prep->map_stage.p, prep->map_stage.p + n, w, h, prep->rec_pitch, prep->rec_xy[camera].p, prep->rec_frac[camera].p, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(stream_wait_blocking(st));   // the staging is free for the other camera, the caller's maps are no longer read
    prep->maps_set[camera] = true;
    return TC2LI_OK;
}

extern "C" int tc2li_image_prep_batch(tc2li_image_prep* prep, const uint8_t* images, int images_on_device, int n_images, int stride,
                                      size_t image_pitch_bytes, uint8_t* dev_gray, int gray_stride, size_t gray_pitch_bytes, void* stream) {
    if (!prep) { set_error("tc2li_image_prep_batch: null handle"); return TC2LI_ERR_INVALID; }
    const tc2li_image_prep_params& p = prep->prm;
    const int rc = validate_call("tc2li_image_prep_batch", p, images, n_images, stride, dev_gray, gray_stride, gray_pitch_bytes);
    if (rc < 0) return rc;
    if (n_images > prep->max_images) {
        set_error("tc2li_image_prep_batch: %d images, the handle was made for %d", n_images, prep->max_images);
        return TC2LI_ERR_CAPACITY;
    }
    std::lock_guard<std::mutex> lk(prep->mu);
    if (p.mode == TC2LI_IMAGE_PREP_RECTIFY && !(prep->maps_set[0] && prep->maps_set[1])) {
        set_error("tc2li_image_prep_batch: mode RECTIFY before tc2li_image_prep_set_maps of both cameras");
        return TC2LI_ERR_INVALID;
    }
    if (n_images == 0) return 0;
    hipStream_t st = (hipStream_t)stream;   // NULL is the null stream here: the extractor's call that follows is ordered behind this one on it
    ImagePrepBatch B{};
    B.src = images; B.src_pitch = image_pitch_bytes; B.src_stride = stride;
    if (!images_on_device) {
        // image by image into pinned memory, rows as they are, then one upload
        const size_t one = image_bytes(p.src_height, stride, p.src_width * p.channels), pitch = align256(one);
        TC2LI_HIP_CHECK(prep->stage.ensure(pitch * (size_t)n_images));
        TC2LI_HIP_CHECK(prep->h_stage.ensure(pitch * (size_t)n_images));
        uint8_t* hs = prep->h_stage.p;
        global_pool().parallel_for(n_images, [&](int i) { memcpy(hs + (size_t)i * pitch, images + (size_t)i * image_pitch_bytes, one); });
        TC2LI_HIP_CHECK(hipMemcpyAsync(prep->stage.p, hs, pitch * (size_t)(n_images - 1) + one, hipMemcpyHostToDevice, st));
        B.src = prep->stage.p; B.src_pitch = pitch;
    }
    B.dst = dev_gray; B.dst_pitch = gray_pitch_bytes; B.dst_stride = gray_stride;
    B.sw = p.src_width; B.sh = p.src_height; B.dw = p.dst_width; B.dh = p.dst_height;
    B.n_images = n_images;
    B.k0 = p.rgb ? prep::kR2Y : prep::kB2Y; B.k2 = p.rgb ? prep::kB2Y : prep::kR2Y;
    if (p.mode == TC2LI_IMAGE_PREP_RECTIFY) {
        for (int cam = 0; cam < 2; ++cam) { B.rec_xy[cam] = prep->rec_xy[cam].p; B.rec_frac[cam] = prep->rec_frac[cam].p; }
        B.rec_pitch = prep->rec_pitch;
        launch_image_prep_rectify(B, p.channels, st);
        TC2LI_HIP_CHECK(hipEventRecord(prep->records_read, st));
        prep->records_in_use = true;
    } else if (p.mode == TC2LI_IMAGE_PREP_RESIZE) {
        B.xofs = prep->xofs.p; B.ialpha = prep->ialpha.p; B.yofs = prep->yofs.p; B.ibeta = prep->ibeta.p;
        launch_image_prep_resize(B, p.channels, st);
    } else {
        launch_image_prep_gray(B, p.channels, st);
    }
    TC2LI_HIP_CHECK(hipGetLastError());
    if (!images_on_device) TC2LI_HIP_CHECK(stream_wait_blocking(st));   // the staging is the next call's
    return n_images;
}

extern "C" int tc2li_host_image_prep_batch(const tc2li_image_prep_params* params, const float* const maps[4], const uint8_t* images, int n_images,
                                           int stride, size_t image_pitch_bytes, uint8_t* gray, int gray_stride, size_t gray_pitch_bytes) {
    const char* entry = "tc2li_host_image_prep_batch";
    int rc = validate_params(entry, params);
    if (rc < 0) return rc;
    rc = validate_call(entry, *params, images, n_images, stride, gray, gray_stride, gray_pitch_bytes);
    if (rc < 0) return rc;
    const tc2li_image_prep_params& p = *params;
    if (p.mode == TC2LI_IMAGE_PREP_RECTIFY) {
        if (!maps || !maps[0] || !maps[1] || !maps[2] || !maps[3]) {
            set_error("%s: mode RECTIFY without the maps of both cameras", entry);
            return TC2LI_ERR_INVALID;
        }
        for (int m = 0; m < 4; ++m)
            if (!map_ok(maps[m], p.dst_width, p.dst_height)) {
                set_error("%s: map %d: a value that is not finite or not below 2^24 in magnitude", entry, m);
                return TC2LI_ERR_INVALID;
            }
    }
    if (n_images == 0) return 0;
    HostJob J;
    J.p = params; J.maps = maps; J.images = images; J.image_pitch = image_pitch_bytes; J.stride = stride;
    J.gray = gray; J.gray_pitch = gray_pitch_bytes; J.gray_stride = gray_stride;
    J.k0 = p.rgb ? prep::kR2Y : prep::kB2Y; J.k2 = p.rgb ? prep::kB2Y : prep::kR2Y; J.nc = p.channels == 1 ? 1 : 3;
    if (p.mode == TC2LI_IMAGE_PREP_RESIZE) build_resize_tables(p.src_width, p.src_height, p.dst_width, p.dst_height, J.xofs, J.ialpha, J.yofs, J.ibeta);
    const int blocks = (p.dst_height + kHostRowsPerUnit - 1) / kHostRowsPerUnit;
    const long long units = (long long)n_images * blocks;
    if (units > 0x7fffffffLL) { set_error("%s: too many rows for one call; split the batch", entry); return TC2LI_ERR_INVALID; }
    global_pool().parallel_for((int)units, [&](int u) {
        const int img = u / blocks, y0 = (u - img * blocks) * kHostRowsPerUnit, y1 = std::min(y0 + kHostRowsPerUnit, p.dst_height);
        for (int y = y0; y < y1; ++y) host_row(J, img, y);
    });
    return n_images;
}
