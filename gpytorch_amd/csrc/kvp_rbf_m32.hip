#define GPAMD_KA gpamd::KIND_RBF
#define GPAMD_KB gpamd::KIND_MATERN32
#define GPAMD_NAME rbf_m32
#include "kvp_family.inc"
