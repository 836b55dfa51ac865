// Stand-alone replay of the ONNX reader (csrc/onnx_graph.cpp) on hostile input, built by tests/test_onnx_cpu.py with a plain g++
// under -fsanitize=address,undefined together with onnx_graph.cpp and ncnn_graph.cpp: host code only, no HIP, no Python.
//
//   onnx_parse_replay <model.onnx>
//
// 1. the file itself lowers to a graph (printed: layers, convolutions);
// 2. every prefix of it in 997-byte steps is refused with LP_ERR_GRAPH -- the reader never reads past the end it was given
//    (each prefix is parsed from a heap copy of exactly that length, so AddressSanitizer sees one byte too many);
// 3. 2000 seeded single-byte corruptions each return normally or throw lp::Error; nothing else escapes.
// Exit status 0 and "replay OK" on success; the sanitizers abort on a finding.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>

#include "../../yolo-litepi_amd/csrc/onnx_graph.h"

namespace lp {
void set_last_error(const std::string&) {}
}  // namespace lp

// parse a heap copy of exactly n bytes; returns 0 when it lowered, else the lp::Error code
static int parse_copy(const std::vector<unsigned char>& file, size_t n, const unsigned char* patch_at = nullptr, size_t at = 0, size_t* layers = nullptr) {
  std::unique_ptr<unsigned char[]> copy(new unsigned char[n ? n : 1]);
  if (n) memcpy(copy.get(), file.data(), n);
  if (patch_at) copy[at] = *patch_at;
  try {
    const lp::NcnnGraph g = lp::onnx_to_graph(copy.get(), n, "replay");
    if (layers) *layers = g.layers.size();
    (void)g.describe();
    return 0;
  } catch (const lp::Error& e) {
    return e.code;
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s model.onnx\n", argv[0]); return 2; }
  std::ifstream f(argv[1], std::ios::binary);
  std::vector<unsigned char> file((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  if (file.empty()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }

  size_t layers = 0;
  const int rc = parse_copy(file, file.size(), nullptr, 0, &layers);
  if (rc != 0 || layers < 100) { fprintf(stderr, "the intact file: status %d, %zu layers\n", rc, layers); return 1; }
  try {
    (void)lp::onnx_file_to_graph(std::string(argv[1]) + ".missing");
    fprintf(stderr, "a missing file was read\n");
    return 1;
  } catch (const lp::Error& e) {
    if (e.code != LP_ERR_IO) { fprintf(stderr, "a missing file gives status %d\n", e.code); return 1; }
  }

  size_t prefixes = 0;
  for (size_t n = 0; n < file.size(); n += 997, ++prefixes) {
    const int c = parse_copy(file, n);
    if (c != LP_ERR_GRAPH) { fprintf(stderr, "prefix of %zu bytes: status %d, LP_ERR_GRAPH expected\n", n, c); return 1; }
  }

  unsigned long long s = 0x9E3779B97F4A7C15ull;   // splitmix64
  auto next = [&s] {
    unsigned long long z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  int ok = 0, refused = 0;
  for (int k = 0; k < 2000; ++k) {
    // half of the corruptions go to the first 32 KB and the last 4 KB, where the structure is densest (nodes, attributes, the
    // small constants); the rest anywhere (mostly weights, which any value leaves valid)
    size_t at = (size_t)(next() % file.size());
    if (k % 2 == 0) at = k % 4 == 0 ? at % std::min<size_t>(file.size(), 32768) : file.size() - 1 - at % std::min<size_t>(file.size(), 4096);
    unsigned char v = (unsigned char)next();
    if (v == file[at]) v ^= 0x80;
    const int c = parse_copy(file, file.size(), &v, at);
    if (c == 0) ++ok;
    else if (c == LP_ERR_GRAPH) ++refused;
    else { fprintf(stderr, "corruption %d (byte %zu = %u): status %d\n", k, at, v, c); return 1; }
  }
  printf("replay OK: %zu layers, %zu prefixes refused, 2000 corruptions: %d lowered, %d refused\n", layers, prefixes, ok, refused);
  return 0;
}
