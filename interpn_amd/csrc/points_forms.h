// What the point-major translation units share (linear_points.h, points_grad.h): the launch-uniform forms of the row
// accesses and the row length up to which the split path's kernels go through their LDS tile.
#pragma once

#include <cstddef>

namespace interpn {

enum PointsLoad : int { kPointsLoadElem = 0, kPointsLoadWide = 1, kPointsLoadLds = 2 };
enum PointsStore : int { kPointsStoreElem = 0, kPointsStoreWide = 1, kPointsStoreLds = 2 };

// Row strides (elements) up to which the fused multilinear gradient kernel takes a block: it addresses a workgroup's rows with
// 32-bit offsets from a uniform base (512 rows at most).  Longer rows go through the split path.
constexpr size_t kPointsGradMaxStride = (size_t)1 << 20;

constexpr size_t kSplitTileStride = 32;  // rows up to this many elements go through the LDS tile

}  // namespace interpn
