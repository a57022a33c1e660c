// sph_encoder_api.hpp -- what the two frame encoders behind the C-ABI (SphPng, SphVideo) share on the host: a file is a fixed header built
// at creation, a payload the device writes and a count pass sizes, and a fixed trailer; a frame comes from a host image or lies in a
// renderer.  Host code, included by sph_api.hip behind sph_render_api.hpp and before the two encoders; `who` is the calling function's
// name in the messages.
#pragma once

struct FrameEncoder : DevObj {   // clk[0]: the stages of an encode
    int W = 0, H = 0;
    std::vector<uint8_t> header, trailer;   // before and behind the payload
    bool have_frame = false;
    int64_t payload_bytes = 0;              // what the device wrote of the frame held
    const unsigned char *src = nullptr;     // the device image the passes of this encode read
    DevBuf rgb, out;                        // a host image's staging; the payload
};

static const char *enc_check_size(int w, int h) {
    if (w < 1 || h < 1 || w > 16384 || h > 16384 || (int64_t)w * h > ((int64_t)1 << 26))
        return "width and height are 1..16384 each, at most 2^26 pixels in all";
    return nullptr;
}

static int enc_no_room(const FrameEncoder *v, const char *who) {
    return fail(nullptr, SPH_ERR_HIP, "%s: buffers of a %d x %d frame", who, v->W, v->H);
}

// stream, clocks and staging buffer of a new encoder; after a failure, here or in the create that called, the object is destroyed
static int enc_open(FrameEncoder *v, const char *who, int w, int h, int dev, bool fast_math) {
    v->W = w; v->H = h;
    const int rc = devobj_open(v, who, dev, fast_math);
    if (rc && !v->stream) return rc;
    if (rc || v->rgb.reserve(nullptr, (size_t)w * h * 3)) return enc_no_room(v, who);
    return SPH_OK;
}

static void enc_close(FrameEncoder *v, DevBuf *buf, int nbuf) {
    devobj_close(v, buf, nbuf);
    v->rgb.release(); v->out.release();
}

// the opening of an encode: the frame held goes, stage mark 0, src on its way (a host image) or complete (a renderer's, read in place:
// nothing of the renderer is written)
static int enc_begin_rgb(FrameEncoder *v, const char *who, const uint8_t *rgb) {
    if (!v) return SPH_ERR_INVALID;
    if (!rgb) return fail(v, SPH_ERR_INVALID, "%s: null image", who);
    HIPCHK(v, hipSetDevice(v->device));
    v->have_frame = false;
    HIPCHK(v, v->clk[0].mark(0));
    HIPCHK(v, hipMemcpyAsync(v->rgb.p, rgb, (size_t)v->W * v->H * 3, hipMemcpyHostToDevice, v->stream));
    v->src = (const unsigned char *)v->rgb.p;
    return SPH_OK;
}

static int enc_begin_render(FrameEncoder *v, const char *who, SphRender *r) {
    if (!v || !r) return SPH_ERR_INVALID;
    { int rc = rend_frame_rgb(r, v->W, v->H, v->device, v, who, &v->src); if (rc) return rc; }
    v->have_frame = false;
    HIPCHK(v, v->clk[0].mark(0));
    return SPH_OK;
}

// between the count pass and the write pass: the output holds exactly the payload -- what the count pass found and `extra` bytes of the
// format's own -- grown with some room so that frames of similar size reuse it
static int enc_room(FrameEncoder *v, int64_t counted, int64_t extra) {
    v->payload_bytes = counted + extra;
    return v->out.reserve(v, (size_t)v->payload_bytes + (size_t)counted / 4 + 64);
}

static int64_t enc_file_bytes(const FrameEncoder *v) { return (int64_t)(v->header.size() + v->trailer.size()) + v->payload_bytes; }

static int enc_size(FrameEncoder *v, const char *who, int64_t *bytes) {
    if (!v || !bytes) return SPH_ERR_INVALID;
    if (!v->have_frame) return fail(v, SPH_ERR_INVALID, "%s: no frame has been encoded yet", who);
    *bytes = enc_file_bytes(v);
    return SPH_OK;
}

static int enc_download(FrameEncoder *v, const char *who, uint8_t *dst) {
    if (!v || !dst) return SPH_ERR_INVALID;
    if (!v->have_frame) return fail(v, SPH_ERR_INVALID, "%s: no frame has been encoded yet", who);
    HIPCHK(v, hipSetDevice(v->device));
    const size_t nh = v->header.size();
    memcpy(dst, v->header.data(), nh);
    HIPCHK(v, hipMemcpy(dst + nh, v->out.p, (size_t)v->payload_bytes, hipMemcpyDeviceToHost));
    memcpy(dst + nh + v->payload_bytes, v->trailer.data(), v->trailer.size());
    return SPH_OK;
}
