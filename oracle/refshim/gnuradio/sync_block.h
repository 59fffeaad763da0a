/* Stand-in for <gnuradio/sync_block.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc): a block whose work() the driver calls. */
#ifndef REFSHIM_GNURADIO_SYNC_BLOCK_H
#define REFSHIM_GNURADIO_SYNC_BLOCK_H
#include <gnuradio/block.h>

namespace gr {

class sync_block : public block {
public:
    sync_block() {}
    sync_block(const std::string &name, io_signature::sptr in, io_signature::sptr out) : block(name, in, out) {}
    virtual int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) = 0;
};

}  // namespace gr

#endif
