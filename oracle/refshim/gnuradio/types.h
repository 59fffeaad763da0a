/* Stand-in for <gnuradio/types.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc).  The item-vector typedefs, boost::shared_ptr
 * mapped to std::, and the C headers the GNU Radio headers pull in for their users (assert, printf, u_int64_t). */
#ifndef REFSHIM_GNURADIO_TYPES_H
#define REFSHIM_GNURADIO_TYPES_H
#include <sys/types.h>
#include <assert.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

namespace boost {
using std::shared_ptr;
}

typedef std::vector<int> gr_vector_int;
typedef std::vector<const void *> gr_vector_const_void_star;
typedef std::vector<void *> gr_vector_void_star;

#endif
