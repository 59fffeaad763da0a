/* Stand-in for <gnuradio/attributes.h> -- TEST INFRASTRUCTURE ONLY (oracle/refdriver.cc): symbols need no visibility mark in one program. */
#ifndef REFSHIM_GNURADIO_ATTRIBUTES_H
#define REFSHIM_GNURADIO_ATTRIBUTES_H
#define __GR_ATTR_EXPORT
#define __GR_ATTR_IMPORT
#endif
