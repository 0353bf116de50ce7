#define GPAMD_SM_D 3
#define GPAMD_SM_Q0 1
#define GPAMD_NAME d3
#include "kvsm_family.inc"
