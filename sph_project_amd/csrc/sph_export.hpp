// sph_export.hpp -- frame export on the host: the ASCII PLY the reference writes per fluid object and frame
// (run_simulation.py:137-144: ti.tools.PLYWriter(num_vertices).add_vertex_pos(x, y, z).export_ascii(path)).  Plain C++ behind the C-ABI
// (included by sph_api.hip; host code only).  Layout restated from Taichi's python/taichi/tools/ply.py (not compared with a Taichi run: the
// package is absent): header "ply / format ascii 1.0 / comment created by PLYWriter / element vertex N / property float x|y|z /
// end_header", then per vertex every value as str(np.float32) followed by ONE blank, "\n" at the end of the line.
// Why native: numpy needs ~5 s to turn the 1.23 M positions of a frame into those strings (it was the 68 ms/step "all in" of the
// reference's final_scene0 in round 3); this writes the same bytes in ~0.2 s.
#pragma once
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>

namespace sphexp {

// str(np.float32(v)): the shortest digits that round-trip (std::to_chars, like numpy's dragon4 in unique mode), positional with at least
// one digit behind the point for 0 and 1e-4 <= |v| < 1e16 ("0.1", "123456790.0", "-0.0"), else scientific with a two-digit exponent
// ("1e-05", "1.2345679e+16"); "inf" / "nan" as numpy prints them.  Returns the number of characters written (no terminator).
static inline int format_f32(float v, char *out) {
    char *p = out;
    if (std::isnan(v)) { memcpy(p, "nan", 3); return 3; }
    if (std::signbit(v)) { *p++ = '-'; v = -v; }
    if (std::isinf(v)) { memcpy(p, "inf", 3); return (int)(p - out) + 3; }
    if (v == 0.0f) { memcpy(p, "0.0", 3); return (int)(p - out) + 3; }
    char sci[48];
    const auto r = std::to_chars(sci, sci + sizeof(sci), v, std::chars_format::scientific);   // d[.ddd]e[+-]XX
    const int len = (int)(r.ptr - sci);
    *r.ptr = 0;   // (atoi below)
    const double a = (double)v;
    if (!(a < 1.e16 && a >= 1.e-4)) { memcpy(p, sci, (size_t)len); return (int)(p - out) + len; }
    int epos = 0;
    while (sci[epos] != 'e') ++epos;
    const int exp10 = atoi(sci + epos + 1);
    char dig[16]; int nd = 0;
    for (int k = 0; k < epos; ++k) if (sci[k] != '.') dig[nd++] = sci[k];
    if (exp10 >= 0) {
        for (int k = 0; k <= exp10; ++k) *p++ = k < nd ? dig[k] : '0';
        *p++ = '.';
        if (nd > exp10 + 1) for (int k = exp10 + 1; k < nd; ++k) *p++ = dig[k];
        else *p++ = '0';
    } else {
        *p++ = '0'; *p++ = '.';
        for (int k = 0; k < -exp10 - 1; ++k) *p++ = '0';
        for (int k = 0; k < nd; ++k) *p++ = dig[k];
    }
    return (int)(p - out);
}

// one part of a PLY: first != 0 truncates the file and writes the header for n_total vertices before this part's n rows, else the rows
// are appended.  Parts in any split give the bytes of the one-shot writer (first = 1, n_total = n).
static int write_ply_ascii_part(const char *path, const float *xyz, int64_t n, int64_t n_total, int first) {
    if (!path || n < 0 || n_total < 0 || n > n_total || (n > 0 && !xyz)) return -1;
    FILE *f = fopen(path, first ? "wb" : "ab");
    if (!f) return -2;
    int rc = 0;
    if (first && fprintf(f, "ply\nformat ascii 1.0\ncomment created by PLYWriter\nelement vertex %lld\nproperty float x\nproperty float y\nproperty float z\nend_header\n", (long long)n_total) < 0) rc = -3;
    std::vector<char> buf(1 << 20);
    size_t used = 0;
    for (int64_t i = 0; i < n && rc == 0; ++i) {
        if (used + 3 * 48 + 4 > buf.size()) { if (fwrite(buf.data(), 1, used, f) != used) rc = -3; used = 0; }
        for (int c = 0; c < 3; ++c) { used += (size_t)format_f32(xyz[3 * i + c], buf.data() + used); buf[used++] = ' '; }
        buf[used++] = '\n';
    }
    if (rc == 0 && used && fwrite(buf.data(), 1, used, f) != used) rc = -3;
    if (fclose(f) != 0 && rc == 0) rc = -3;
    return rc;
}

static int write_ply_ascii(const char *path, const float *xyz, int64_t n) { return write_ply_ascii_part(path, xyz, n, n, 1); }

// one reconstructed surface as ASCII OBJ: "v x y z" per vertex, "vn x y z" per normal, "f a//a b//b c//c" (1-based; "f a b c" without
// normals) per triangle, numbers as format_f32
static int write_obj_ascii(const char *path, const float *v, int64_t nv, const float *nrm, const int32_t *tri, int64_t nt) {
    if (!path || nv < 0 || nt < 0 || (nv > 0 && !v) || (nt > 0 && !tri)) return -1;
    for (int64_t k = 0; k < 3 * nt; ++k) if (tri[k] < 0 || tri[k] >= nv) return -1;
    FILE *f = fopen(path, "wb");
    if (!f) return -2;
    int rc = 0;
    std::vector<char> buf(1 << 20);
    size_t used = 0;
    auto flush = [&](size_t room) {
        if (used + room > buf.size()) { if (fwrite(buf.data(), 1, used, f) != used) rc = -3; used = 0; }
    };
    for (int pass = 0; pass < 2; ++pass) {
        const float *a = pass == 0 ? v : nrm;
        if (!a) continue;
        for (int64_t i = 0; i < nv && rc == 0; ++i) {
            flush(3 * 48 + 8);
            buf[used++] = 'v';
            if (pass == 1) buf[used++] = 'n';
            for (int c = 0; c < 3; ++c) { buf[used++] = ' '; used += (size_t)format_f32(a[3 * i + c], buf.data() + used); }
            buf[used++] = '\n';
        }
    }
    for (int64_t i = 0; i < nt && rc == 0; ++i) {
        flush(3 * 48 + 8);
        buf[used++] = 'f';
        for (int c = 0; c < 3; ++c) {
            const long long k = (long long)tri[3 * i + c] + 1;
            used += (size_t)(nrm ? snprintf(buf.data() + used, 48, " %lld//%lld", k, k) : snprintf(buf.data() + used, 48, " %lld", k));
        }
        buf[used++] = '\n';
    }
    if (rc == 0 && used && fwrite(buf.data(), 1, used, f) != used) rc = -3;
    if (fclose(f) != 0 && rc == 0) rc = -3;
    return rc;
}

}  // namespace sphexp
