#define GPAMD_KB gpamd::KIND_MATERN52
#define GPAMD_NAME matern52
#include "kvn_family.inc"
