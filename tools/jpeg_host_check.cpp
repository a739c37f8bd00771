// The host stage of the JPEG decode (csrc/jpeg.hip: marker parsing + entropy decoding) under the host
// sanitizers, stand-alone: no Python, no device call.  tools/jpeg_host_check.sh builds it together with
// jpeg.hip (-Xarch_host -fsanitize=address,undefined) and feeds it the files `tests/jpeg_cases.py --dump`
// writes.  For every file, vcap_jpeg_header and vcap_jpeg_host_stage see, each time from a heap buffer of
// exactly the input's size (so one byte read past the end is an AddressSanitizer report):
//   1. every prefix of the file (and the file itself);
//   2. every header byte (all bytes up to the entropy-coded data) replaced by 0x00, by 0xFF, by the byte + 1
//      and by the byte - 1;
//   3. every 16th byte of the entropy-coded data replaced by 0xFF, by FF D9 and by FF D0.
// The enumeration is fixed: the same calls on every run.  Every call has to return 0, VCAP_E_ARG or
// VCAP_E_UNSUPPORTED, and both entry points have to agree.  -DJPEG_HOST_CHECK_HEADER_ONLY leaves the host stage
// out, for a jpeg.hip from before it was split off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/vcap.h"
#include "vcap_kernels.h"

namespace {

long g_calls = 0, g_accepted = 0, g_arg = 0, g_unsupported = 0;

void fail(const char* file, const char* what, size_t at, int rc, const std::string& err) {
  std::fprintf(stderr, "FAIL %s: %s at %zu: rc %d (%s)\n", file, what, at, rc, err.c_str());
  std::exit(1);
}

void run(const char* file, const char* what, size_t at, const uint8_t* bytes, size_t len) {
  uint8_t* data = new uint8_t[len];  // exactly len bytes: nothing readable behind them
  std::memcpy(data, bytes, len);
  JpegInfo info;
  std::string err;
  const int rc = vcap_jpeg_header(data, len, &info, &err);
  if (rc != 0 && rc != VCAP_E_ARG && rc != VCAP_E_UNSUPPORTED) fail(file, what, at, rc, err);
#ifndef JPEG_HOST_CHECK_HEADER_ONLY
  std::vector<char> stage;
  JpegInfo staged;
  std::string err2;
  const uint8_t* one = data;
  const int rc2 = vcap_jpeg_host_stage(
      &one, &len, 1, &staged,
      [&](const JpegInfo&, size_t bytes_needed, int*, std::string*) -> void* {
        stage.assign(bytes_needed ? bytes_needed : 1, 0);
        return stage.data();
      },
      &err2);
  if (rc2 != rc) fail(file, what, at, rc2, "host stage disagrees with the header: " + err2);
  if (rc2 == 0 && (staged.width != info.width || staged.height != info.height || staged.ncomp != info.ncomp))
    fail(file, what, at, rc2, "host stage reports another shape");
#endif
  ++g_calls;
  (rc == 0 ? g_accepted : rc == VCAP_E_ARG ? g_arg : g_unsupported)++;
  delete[] data;
}

// offset of the entropy-coded data (behind the SOS segment), or the file's length when there is no SOS
size_t scan_start(const std::vector<uint8_t>& f) {
  size_t i = 2;
  while (i + 4 <= f.size()) {
    if (f[i] != 0xFF) return f.size();
    while (i < f.size() && f[i] == 0xFF) ++i;
    if (i + 2 >= f.size()) return f.size();
    const int m = f[i++];
    const size_t n = ((size_t)f[i] << 8) | f[i + 1];
    if (n < 2 || i + n > f.size()) return f.size();
    if (m == 0xDA) return i + n;
    i += n;
  }
  return f.size();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: jpeg_host_check FILE.jpg ...\n");
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    std::FILE* fp = std::fopen(argv[a], "rb");
    if (!fp) {
      std::fprintf(stderr, "cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> f;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), fp)) > 0;) f.insert(f.end(), buf, buf + n);
    std::fclose(fp);
    const char* name = std::strrchr(argv[a], '/') ? std::strrchr(argv[a], '/') + 1 : argv[a];
    const long before = g_calls;
    const size_t head = scan_start(f);
    for (size_t n = 0; n <= f.size(); ++n) run(name, "prefix", n, f.data(), n);
    std::vector<uint8_t> m = f;
    for (size_t k = 0; k < head; ++k) {
      const uint8_t b = f[k];
      for (const uint8_t v : {(uint8_t)0x00, (uint8_t)0xFF, (uint8_t)(b + 1), (uint8_t)(b - 1)}) {
        m[k] = v;
        run(name, "header byte", k, m.data(), m.size());
      }
      m[k] = b;
    }
    for (size_t k = head; k < f.size(); k += 16) {
      const uint8_t b0 = f[k], b1 = k + 1 < f.size() ? f[k + 1] : 0;
      m[k] = 0xFF;
      run(name, "scan byte -> FF", k, m.data(), m.size());
      for (const uint8_t second : {(uint8_t)0xD9, (uint8_t)0xD0}) {
        if (k + 1 < f.size()) m[k + 1] = second;
        run(name, second == 0xD9 ? "scan bytes -> FF D9" : "scan bytes -> FF D0", k, m.data(), m.size());
      }
      m[k] = b0;
      if (k + 1 < f.size()) m[k + 1] = b1;
    }
    std::printf("%-48s %6zu bytes, header %5zu: %6ld calls\n", name, f.size(), head, g_calls - before);
  }
  std::printf("%d files, %ld calls: %ld accepted, %ld VCAP_E_ARG, %ld VCAP_E_UNSUPPORTED; no other code, no report\n",
              argc - 1, g_calls, g_accepted, g_arg, g_unsupported);
  return 0;
}
