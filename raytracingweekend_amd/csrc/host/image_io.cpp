// image_io.cpp — the PPM reader behind image_texture (rtw/texture.h).
//
// The reference's image_texture takes its pixels from the caller and ships no
// loader; this one reads the format the renderer itself writes (P3, rows top
// to bottom: RayTracingWeekend.cpp:252-276) and its binary sibling P6.
// Host code only.
#include <cstdio>
#include <string>
#include <vector>
#include "rtw/texture.h"
#include "rtw_host_util.h"

namespace {

struct reader {
    const std::vector<unsigned char>& b;
    size_t at = 0;

    // skip white space and '#' comments (to the end of their line)
    void skip() {
        while (at < b.size()) {
            const unsigned char c = b[at];
            if (c == '#') {
                while (at < b.size() && b[at] != '\n') ++at;
            } else if (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v') {
                ++at;
            } else {
                break;
            }
        }
    }
    // one unsigned decimal number of at most 9 digits; false when none is here
    bool number(long& out) {
        skip();
        size_t n = 0;
        long v = 0;
        while (at < b.size() && b[at] >= '0' && b[at] <= '9') {
            if (++n > 9) return false;
            v = v * 10 + (b[at++] - '0');
        }
        out = v;
        return n > 0;
    }
};

}  // namespace

int rtw_load_ppm(const std::string& path, image_texture::byte_array& pixels, int& nx, int& ny) {
    pixels.clear();
    nx = ny = 0;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: cannot open " + path);
    std::vector<unsigned char> buf;
    unsigned char chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool read_error = std::ferror(f) != 0;
    std::fclose(f);
    if (read_error) return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: read error in " + path);

    if (buf.size() < 2 || buf[0] != 'P' || (buf[1] != '6' && buf[1] != '3'))
        return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + " is neither a P6 nor a P3 PPM (bad magic)");
    const bool binary = buf[1] == '6';
    reader r{buf, 2};
    long w = 0, h = 0, maxval = 0;
    if (!r.number(w) || !r.number(h) || !r.number(maxval))
        return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": malformed header");
    if (w < 1 || h < 1 || w > (1 << 24) || h > (1 << 24))
        return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": image size out of range");
    if (maxval != 255)
        return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": maxval " + std::to_string(maxval) +
                                             " (only 255 is supported)");
    const unsigned long long need = 3ull * (unsigned long long)w * (unsigned long long)h;
    if (need > (1ull << 31) - 1) return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": image too large");
    if (binary) {
        // exactly one white-space byte separates maxval from the raster
        if (r.at >= buf.size() || !(buf[r.at] == ' ' || buf[r.at] == '\t' || buf[r.at] == '\n' || buf[r.at] == '\r'))
            return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": malformed header");
        ++r.at;
        if (buf.size() - r.at < need) return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": truncated raster");
        pixels.assign(buf.begin() + r.at, buf.begin() + r.at + need);
    } else {
        pixels.reserve(need);
        for (unsigned long long k = 0; k < need; ++k) {
            long v;
            if (!r.number(v)) {
                pixels.clear();
                return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": truncated or malformed raster");
            }
            if (v > 255) {
                pixels.clear();
                return rtw_fail(RTW_ERR_INVALID, "rtw_load_ppm: " + path + ": sample above maxval");
            }
            pixels.push_back((unsigned char)v);
        }
    }
    nx = (int)w;
    ny = (int)h;
    return RTW_OK;
}
