#include "ref_shim.h"  // stand-in: everything the kernel files use of this header is emulated there
