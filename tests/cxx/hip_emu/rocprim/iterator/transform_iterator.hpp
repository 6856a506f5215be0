#pragma once
#include <rocprim/device/device_scan.hpp>
