#define GPAMD_KB gpamd::KIND_MATERN32
#define GPAMD_NAME matern32
#include "kva_family.inc"
