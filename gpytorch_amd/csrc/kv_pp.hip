#define GPAMD_KIND gpamd::KIND_PP
#define GPAMD_NAME pp
#include "kv_family.inc"
