// What data_feed.hip shares with image_feed.hip: the one table of ToTensor + Normalize(0.5, 0.5) values (kFetchTable).
#pragma once
#include <hip/hip_runtime.h>

namespace diagan {

// *table = the 256 floats of kFetchTable on the current device (device memory; a lookup, no launch and no synchronisation)
hipError_t fetch_table_device(const float** table);

}  // namespace diagan
