#define GPAMD_KA gpamd::KIND_MATERN32
#define GPAMD_KB gpamd::KIND_MATERN32
#define GPAMD_NAME m32_m32
#include "kvp_family.inc"
