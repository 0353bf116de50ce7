#define GPAMD_KB gpamd::KIND_MATERN12
#define GPAMD_NAME matern12
#include "kvt_family.inc"
