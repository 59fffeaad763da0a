/* Stand-in for <gnuradio/block.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc).  A block here has no scheduler: its ports
 * record what is published, set_msg_handler stores the handler for the driver to call, consume_each does nothing. */
#ifndef REFSHIM_GNURADIO_BLOCK_H
#define REFSHIM_GNURADIO_BLOCK_H
#include <functional>
#include <map>
#include <utility>
#include <boost/bind.hpp>
#include <gnuradio/io_signature.h>
#include <pmt/pmt.h>

namespace gr {

class block {
public:
    typedef std::function<void(pmt::pmt_t)> msg_handler_t;
    /* (port name, message) in the order published; the driver reads and clears it */
    std::vector<std::pair<std::string, pmt::pmt_t> > published;
    std::map<std::string, msg_handler_t> handlers;

    block() {}
    block(const std::string &name, io_signature::sptr, io_signature::sptr) : d_name(name) {}
    virtual ~block() {}

    void message_port_register_in(pmt::pmt_t) {}
    void message_port_register_out(pmt::pmt_t) {}
    void message_port_pub(pmt::pmt_t port, pmt::pmt_t msg) { published.push_back(std::make_pair(port->text, msg)); }
    template <typename T>
    void set_msg_handler(pmt::pmt_t port, T handler) { handlers[port->text] = msg_handler_t(handler); }
    void consume_each(int) {}

    virtual void forecast(int, gr_vector_int &) {}
    virtual int general_work(int, gr_vector_int &, gr_vector_const_void_star &, gr_vector_void_star &) { return 0; }

private:
    std::string d_name;
};

}  // namespace gr

namespace gnuradio {
template <typename T>
boost::shared_ptr<T> get_initial_sptr(T *p) { return boost::shared_ptr<T>(p); }
}  // namespace gnuradio

#endif
