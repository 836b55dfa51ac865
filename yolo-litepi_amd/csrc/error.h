// Errors of liblitepi_hip: the exception every layer throws and the C ABI turns into a status (handle.h LP_API_END).
// Host-pure (no HIP headers): the model readers (ncnn_graph, onnx_graph) build with a plain C++ compiler on top of this alone.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/litepi.h"

namespace lp {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

std::string fmt(const char* f, ...) __attribute__((format(printf, 1, 2)));
inline std::string fmt(const char* f, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof(buf), f, ap);
  va_end(ap);
  return std::string(buf);
}
void set_last_error(const std::string& s);

#define LP_CHECK(cond, code, ...)                                \
  do {                                                           \
    if (!(cond)) throw lp::Error(code, lp::fmt(__VA_ARGS__));    \
  } while (0)

}  // namespace lp
