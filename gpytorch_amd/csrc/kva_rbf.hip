#define GPAMD_KB gpamd::KIND_RBF
#define GPAMD_NAME rbf
#include "kva_family.inc"
