// include/fotg/flowcolor.h -- the reference's flow_code/C colour tool pieces over the C-ABI of libfotg.so:
//   OFC::MotionToColor   color_flow.cpp MotionToColor on the GPU (fotg_flow_color): device flow h x w x 2 -> device RGB h x w x 3,
//                        normalised per image by its largest known motion or by maxmotion > 0; the five printed values on request
//   OFC::ReadFlowFile    flowIO.cpp ReadFlowFile: a Middlebury .flo into a host vector (h x w x 2 float32)
//   OFC::SavePNG         a dependency-free 8-bit RGB PNG writer (stored deflate blocks, CRC-32, Adler-32): no libpng, no zlib
// Plain C++ (no HIP header needed): the device pointers are the caller's.
// Stream-ordered memory (a call without `stats` keeps its per-image keys there): a second call on a stream whose earlier call is
// still pending may wait on the host (include/fotg.h, STREAM-ORDERED MEMORY); the first returns at once.
#ifndef FOTG_OFC_FLOWCOLOR_HEADER
#define FOTG_OFC_FLOWCOLOR_HEADER
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../fotg.h"

namespace OFC {

// flow: n x height x width x 2 float32 (device); rgb: n x height x width x 3 uint8 (device), R, G, B.  maxmotion <= 0: per image,
// as color_flow without its argument.  stats: NULL or n x 5 float32 (DEVICE): maxrad, minu, maxu, minv, maxv.  Asynchronous on
// `stream` (a hipStream_t, 0 = the null stream).  Returns a FOTG_* status.
inline int MotionToColor(const float *flow, int width, int height, unsigned char *rgb, float maxmotion = -1, float *stats = nullptr,
                         int n = 1, int device = 0, void *stream = nullptr)
{
  return fotg_flow_color(device, n, flow, width, height, maxmotion, rgb, stats, stream);
}

// false (and an empty flow) when the file cannot be read or is not a .flo of the reference's format (tag 202021.25, sizes 1..99999)
inline bool ReadFlowFile(std::vector<float> &flow, int &width, int &height, const char *filename)
{
  flow.clear();
  width = height = 0;
  if (!filename) return false;
  const char *dot = strrchr(filename, '.');
  if (!dot || strcmp(dot, ".flo") != 0) return false;
  FILE *f = fopen(filename, "rb");
  if (!f) return false;
  float tag = 0;
  int w = 0, h = 0;
  bool ok = fread(&tag, sizeof(float), 1, f) == 1 && fread(&w, sizeof(int), 1, f) == 1 && fread(&h, sizeof(int), 1, f) == 1 &&
            tag == 202021.25f && w >= 1 && w <= 99999 && h >= 1 && h <= 99999;
  if (ok) {
    flow.resize((size_t)w * h * 2);
    ok = fread(flow.data(), sizeof(float), flow.size(), f) == flow.size();
  }
  fclose(f);
  if (!ok) { flow.clear(); return false; }
  width = w; height = h;
  return true;
}

namespace png_detail {
inline uint32_t crc32(uint32_t crc, const unsigned char *p, size_t n)
{
  crc = ~crc;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
  }
  return ~crc;
}
inline void put32(std::vector<unsigned char> &v, uint32_t x)
{
  for (int s = 24; s >= 0; s -= 8) v.push_back((unsigned char)(x >> s));
}
inline bool chunk(FILE *f, const char *tag, const std::vector<unsigned char> &data)
{
  std::vector<unsigned char> c;
  put32(c, (uint32_t)data.size());
  c.insert(c.end(), tag, tag + 4);
  c.insert(c.end(), data.begin(), data.end());
  put32(c, crc32(0, c.data() + 4, c.size() - 4));
  return fwrite(c.data(), 1, c.size(), f) == c.size();
}
}  // namespace png_detail

// rgb: height x width x 3 uint8 on the HOST, R, G, B.  A zlib stream of stored (uncompressed) deflate blocks: larger files than a
// compressing writer, readable by every PNG decoder.
inline bool SavePNG(const unsigned char *rgb, int width, int height, const char *filename)
{
  using namespace png_detail;
  if (!rgb || !filename || width <= 0 || height <= 0) return false;
  const size_t row = (size_t)width * 3 + 1;
  std::vector<unsigned char> raw(row * height);
  for (int y = 0; y < height; ++y) {
    raw[y * row] = 0;                                            // filter type 0 (none)
    memcpy(&raw[y * row + 1], rgb + (size_t)y * width * 3, (size_t)width * 3);
  }
  std::vector<unsigned char> z = {0x78, 0x01};                   // zlib header: deflate, 32 KiB window, no dictionary
  for (size_t off = 0; off < raw.size() || off == 0;) {
    const size_t len = raw.size() - off < 65535 ? raw.size() - off : 65535;
    const bool last = off + len == raw.size();
    z.push_back(last ? 1 : 0);                                   // BFINAL, BTYPE = 00 (stored)
    z.push_back((unsigned char)(len & 0xff)); z.push_back((unsigned char)(len >> 8));
    z.push_back((unsigned char)(~len & 0xff)); z.push_back((unsigned char)((~len >> 8) & 0xff));
    z.insert(z.end(), raw.begin() + off, raw.begin() + off + len);
    off += len;
    if (last) break;
  }
  uint32_t a = 1, b = 0;                                         // Adler-32 of the uncompressed stream
  for (unsigned char c : raw) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
  put32(z, (b << 16) | a);
  std::vector<unsigned char> ihdr;
  put32(ihdr, (uint32_t)width); put32(ihdr, (uint32_t)height);
  ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});                      // 8 bits, truecolour, deflate, filter 0, no interlace
  FILE *f = fopen(filename, "wb");
  if (!f) return false;
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  bool ok = fwrite(sig, 1, 8, f) == 8 && chunk(f, "IHDR", ihdr) && chunk(f, "IDAT", z) && chunk(f, "IEND", {});
  return (fclose(f) == 0) && ok;
}

}  // namespace OFC
#endif
