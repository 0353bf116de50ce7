#define GPAMD_KB gpamd::KIND_MATERN32
#define GPAMD_NAME matern32
#include "kvt_family.inc"
