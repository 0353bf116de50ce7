#define GPAMD_SM_D 2
#define GPAMD_SM_Q0 1
#define GPAMD_NAME d2
#include "kvsm_family.inc"
