/* Stand-in for <gnuradio/io_signature.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc): the three numbers, kept and never read. */
#ifndef REFSHIM_GNURADIO_IO_SIGNATURE_H
#define REFSHIM_GNURADIO_IO_SIGNATURE_H
#include <gnuradio/types.h>

namespace gr {
class io_signature {
public:
    typedef boost::shared_ptr<io_signature> sptr;
    int min_streams, max_streams, item_size;
    static sptr make(int lo, int hi, int size) {
        sptr s(new io_signature());
        s->min_streams = lo;
        s->max_streams = hi;
        s->item_size = size;
        return s;
    }
};
}  // namespace gr

#endif
