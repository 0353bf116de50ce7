#define GPAMD_KB gpamd::KIND_RBF
#define GPAMD_NAME rbf
#include "kvn_family.inc"
