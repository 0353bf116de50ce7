#define GPAMD_SM_D 1
#define GPAMD_SM_Q0 1
#define GPAMD_NAME d1a
#include "kvsm_family.inc"
