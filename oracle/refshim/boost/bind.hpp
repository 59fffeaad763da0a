/* Stand-in for <boost/bind.hpp> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc): boost::bind and the global _1 ... mapped to std::. */
#ifndef REFSHIM_BOOST_BIND_HPP
#define REFSHIM_BOOST_BIND_HPP
#include <functional>

namespace boost {
using std::bind;
}
using namespace std::placeholders;

#endif
