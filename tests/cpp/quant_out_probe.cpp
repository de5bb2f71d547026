// quant_out_probe.cpp — the size classes of CRTHIP_BIND_QUANTIZED from the library's own headers (kernels.h, quant_out.h), for
// tests/quantized_outputs.py.  One query a line on stdin, one answer a line on stdout ("?" for an unknown one):
//   const NAME   -> VALUE     QOUT_BLOB_MAX, QOUT_BLOCK, QOUT_THREADS, QOUT_SPAN_MAX, RECORD_BYTES, JOB_BYTES
#include "kernels.h"
#include "quant_out.h"

#include <iostream>
#include <sstream>
#include <string>

using namespace corto_hip;

int main() {
	std::string line;
	while(std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd, name;
		in >> cmd >> name;
		if(cmd != "const") { std::cout << "?" << std::endl; continue; }
		if(name == "QOUT_BLOB_MAX") std::cout << QOUT_BLOB_MAX << std::endl;
		else if(name == "QOUT_BLOCK") std::cout << QOUT_BLOCK << std::endl;
		else if(name == "QOUT_THREADS") std::cout << QOUT_THREADS << std::endl;
		else if(name == "QOUT_SPAN_MAX") std::cout << QOUT_SPAN_MAX << std::endl;
		else if(name == "RECORD_BYTES") std::cout << sizeof(crthip_quant_transform) << std::endl;
		else if(name == "JOB_BYTES") std::cout << sizeof(QuantOutJob) << std::endl;
		else std::cout << "?" << std::endl;
	}
	return 0;
}
