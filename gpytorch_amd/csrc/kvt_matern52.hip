#define GPAMD_KB gpamd::KIND_MATERN52
#define GPAMD_NAME matern52
#include "kvt_family.inc"
