#define GPAMD_KA gpamd::KIND_RBF
#define GPAMD_KB gpamd::KIND_MATERN52
#define GPAMD_NAME rbf_m52
#include "kvp_family.inc"
