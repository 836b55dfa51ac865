// ONNX reader (host, no protobuf library): walks the wire format of a YOLOv8-family detector export and lowers it to the
// NcnnGraph the planner (detector_plan.cpp) takes, so an .onnx file reaches the same fused launches as its NCNN twin.
// DESIGN.md 6i has the lowering table and what is refused.
#pragma once
#include "ncnn_graph.h"

namespace lp {

// `name` stands for the file in messages.  Throws lp::Error(LP_ERR_GRAPH) for a truncated or malformed file and for every
// node outside the lowering rules (the message names the node and its op); never reads outside [data, data + bytes).
NcnnGraph onnx_to_graph(const void* data, size_t bytes, const std::string& name);
NcnnGraph onnx_file_to_graph(const std::string& path);   // LP_ERR_IO when the file cannot be read

}  // namespace lp
