/* oracle/ref_shim: see ref_tbb_shim.h */
#pragma once
#include "ref_tbb_shim.h"
