// lane_map_driver.cpp — prints the lane -> pixel maps of csrc/lrp_lane_map.h (the header compiles on the host: its
// static_asserts hold when this program builds) for tests/test_lane_map.py: one line per map and lane,
//   <map name> <lane> <service group> <row> <column>
#include <cstdio>

#include "lrp_lane_map.h"

int main() {
  const struct {
    const char *name;
    lrp::WinLaneMap map;
  } maps[] = {{"row_major", lrp::kLaneRowMajor}, {"rows", lrp::kLaneRows}, {"patches", lrp::kLanePatches}};
  for (const auto &m : maps)
    for (int lane = 0; lane < 64; ++lane)
      std::printf("%s %d %d %d %d\n", m.name, lane, lrp::lane_service_group(lane), lrp::lane_pixel_row(m.map, lane), lrp::lane_pixel_col(m.map, lane));
  return 0;
}
