#define GPAMD_SM_D 1
#define GPAMD_SM_Q0 5
#define GPAMD_NAME d1b
#include "kvsm_family.inc"
