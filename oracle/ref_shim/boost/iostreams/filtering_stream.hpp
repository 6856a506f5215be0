/* oracle/ref_shim: empty on purpose -- nothing the reference scorer build compiles uses this header (tests/ref_bridge.py) */
#pragma once
