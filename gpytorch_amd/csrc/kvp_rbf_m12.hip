#define GPAMD_KA gpamd::KIND_RBF
#define GPAMD_KB gpamd::KIND_MATERN12
#define GPAMD_NAME rbf_m12
#include "kvp_family.inc"
