/* Prints the layout of zg_shuffle as the C compiler sees it (tests/test_shuffle_host.py compares it with the ctypes
 * mirror of 0g-halo2_amd/zg_halo2.py and with zg_lookup's).  C99, nothing but the header. */
#include <stddef.h>
#include <stdio.h>

#include "zg_halo2.h"

int main(void) {
    printf("{\"size\": %zu, \"fields\": {\"width\": %zu, \"inputs\": %zu, \"shuffles\": %zu}, \"lookup_size\": %zu, "
           "\"lookup_tables\": %zu, \"max_shuffles\": %d, \"max_width\": %d}\n",
           sizeof(zg_shuffle), offsetof(zg_shuffle, width), offsetof(zg_shuffle, inputs), offsetof(zg_shuffle, shuffles),
           sizeof(zg_lookup), offsetof(zg_lookup, tables), (int)ZG_MAX_SHUFFLES, (int)ZG_MAX_LOOKUP_WIDTH);
    return 0;
}
