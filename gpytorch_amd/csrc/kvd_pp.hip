#define GPAMD_KIND gpamd::KIND_PP
#define GPAMD_NAME pp
#include "kvd_family.inc"
