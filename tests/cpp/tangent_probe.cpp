// tangent_probe.cpp — the size class of crthip_batch_bind_computed_tangents from the library's own headers (batch_internal.h, tangent.h), for
// tests/test_computed_tangents_gpu.py.  One query a line on stdin, one answer a line on stdout ("?" for an unknown one):
//   const NAME   -> VALUE     TANGENT_BLOB_MAX, TAN_BLOCK, TAN_THREADS, TAN_ROUND_FACES, LDS_AT_MAX, JOB_BYTES
#include "batch_internal.h"

#include <iostream>
#include <sstream>
#include <string>

int main() {
	std::string line;
	while(std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd, name;
		in >> cmd >> name;
		if(cmd != "const") { std::cout << "?" << std::endl; continue; }
		if(name == "TANGENT_BLOB_MAX") std::cout << TANGENT_BLOB_MAX << std::endl;
		else if(name == "TAN_BLOCK") std::cout << TAN_BLOCK << std::endl;
		else if(name == "TAN_THREADS") std::cout << TAN_THREADS << std::endl;
		else if(name == "TAN_ROUND_FACES") std::cout << TAN_ROUND*TAN_THREADS << std::endl;   // faces of one round of k_tangent_blob's workgroup
		else if(name == "LDS_AT_MAX") std::cout << tangent_blob_lds(TANGENT_BLOB_MAX) << std::endl;
		else if(name == "JOB_BYTES") std::cout << sizeof(TangentJob) << std::endl;
		else std::cout << "?" << std::endl;
	}
	return 0;
}
